"""GPU: every kernel, store path and epilogue of csrc/gemm_bf16.hip against the exact references of tests/gemm_cases.py (the method,
the guard bands and the derivation of the activation bounds: its docstring; test_gemm_cases_cpu.py shows that the comparator used
here rejects each defect these kernels could have).

Every test asserts through ma_gemm_bf16_variant / ma_conv1d_taps_bf16_variant - the host query the launch itself switches on - that
its shape ran the kernel it names: a change of the selection thresholds fails here instead of silently un-testing a kernel.

Paths of gemm_store_tile these tests run: the staged bf16 body (ld % 8 == 0, 16-byte base), the lean "inside" body with float32
16-byte and bf16 8-byte stores (OUT == 2: ld % 8 != 0 or a base 8 bytes off), the per-element body (odd ld; the column tile that
crosses N with N % 4 != 0 under bias, ReLU, row_scale, alpha, a residual with ldr % 4 == 0 and odd, in place, the column affine and a
second activation), every one of them on the 64 x 128 (2 and 3 stages), 128 x 128 and both 8-phase kernels; the non-temporal stores of
the tile, 8-phase and weight-stationary kernels; the split-K partial stores with N % 4 != 0.

Float32 activation errors measured on an MI355X against the derived per-element bounds of gemm_cases.act_bound (u = 2^-24; the
same figures on all seven shapes and on both layouts: the pre-activations are integers, so every shape meets the same values):
                                   largest |got - ref| / bound (must be <= 1)      largest |got - ref|
    sigmoid                                 0.464                                   5.47e-08 = 0.92 u
    swish                                   0.443                                   1.13e-06 = 19.0 u  (at a large |y|)
    tanh                                    0.488                                   1.09e-07 = 1.84 u  (bound at y = 0: 5 u)
    ReLU -> affine -> tanh -> row_scale     0.488                                   2.19e-07 = 3.67 u  (row_scale 2 doubles both)
No measurement exceeds its bound; the bounds are about twice what the hardware does (v_exp_f32 and v_rcp_f32 err by less than the
1 ULP the instruction-set guide grants them).  test_epi1 prints these figures on every run (pytest -s).
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TILE_KERNELS = (G.T128X2, G.T64X2, G.T64X3)


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _lib

    assert torch.cuda.is_available()
    return _lib.load()


_cache = {}


def _case(name, act=False):
    """The exact (act=False) or the activation case of a named shape, on the device, built once."""
    key = (name, act)
    if key not in _cache:
        shapes = dict(G.KERNEL_SHAPES)
        shapes.update(G.NT_SHAPES)
        _, M, N, K = shapes[name]
        c = G.Case(M, N, K, density=G.act_density(K), seed=2, hot=False) if act else G.Case(M, N, K, seed=1)
        _cache[key] = c.to(DEV)
    return _cache[key]


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr())


def _stream():
    from mindaudio_amd import _host

    return _host.current_stream_ptr()


def _epilogue(c, name, out_dtype, residual=None):
    from mindaudio_amd import _lib

    spec = G.EPILOGUES[name]
    e = _lib.GemmEpilogue()
    e.alpha = float(spec.get("alpha", 1.0))
    e.act, e.act2 = spec.get("act", 0), spec.get("act2", 0)
    e.out_bf16 = 1 if out_dtype == BF16 else 0
    if spec.get("bias"):
        e.bias = c.bias.data_ptr()
    if spec.get("row_scale"):
        e.row_scale = c.row_scale.data_ptr()
    if spec.get("affine"):
        e.col_scale, e.col_shift = c.col_scale.data_ptr(), c.col_shift.data_ptr()
    if spec.get("residual"):
        assert residual is not None and residual.dtype == F32 and residual.stride(1) == 1
        e.residual, e.ldr = residual.data_ptr(), residual.stride(0)
    return e


def _gemm(lib, a, w, win, e, expect_kernel, expect_epi1=None, expect_nt=None):
    """Ask the query, launch into the window, return the kernel that ran."""
    M, N, K = win.M, win.N, a.shape[1]
    v = lib.ma_gemm_bf16_variant(M, N, K, win.ld, ctypes.byref(e), _ptr(win.view), 0)
    assert v > 0, v
    if isinstance(expect_kernel, tuple):
        assert v & 0xF in expect_kernel, "ran kernel %d, wanted one of %s" % (v & 0xF, expect_kernel)
    else:
        assert v & 0xF == expect_kernel, "the shape ran kernel %d, not %d: the shape no longer tests its kernel" % (v & 0xF, expect_kernel)
    if expect_epi1 is not None:
        assert bool(v & 0x10) == expect_epi1
    if expect_nt is not None:
        assert bool(v & 0x100) == expect_nt
    rc = lib.ma_gemm_bf16(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(win.view), win.ld, M, N, K, ctypes.byref(e), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return v & 0xF


def _strided(x, ld_extra, off=4):
    """A copy of the (rows, cols) float32 tensor x as a column window of a wider buffer: row stride cols + ld_extra."""
    buf = torch.full((x.shape[0], x.shape[1] + ld_extra), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, off:off + x.shape[1]] = x
    return buf[:, off:off + x.shape[1]]


def _want(ref, dtype):
    return ref.float() if dtype == F32 else ref.float().bfloat16()


# ---- one shape per kernel x the launch matrix -------------------------------------------------------------------------------------------
MATRIX_EPILOGUES = ("none", "bias_relu", "res4", "res_odd", "inplace")


@pytest.mark.parametrize("name", list(G.KERNEL_SHAPES))
def test_launch_matrix(lib, name):
    """float32 / bf16 x four output layouts x {no epilogue, bias + ReLU, bias + row_scale + alpha 0.5 + residual with ldr % 4 == 0, with
    an odd ldr, in place}, and a strided A.  The weight-stationary kernel takes what its dispatch condition admits (bf16, ld % 8 == 0,
    16-byte base, no residual, alpha 1); every other launch of its shapes must fall to a tile kernel and still be exact."""
    kernel = G.KERNEL_SHAPES[name][0]
    c = _case(name)
    tile = G.KERNEL_TILE[kernel]
    z = c.z()
    refs = {k: G.epilogue_ref(z, c, k)[0] for k in ("none", "bias_relu", "bias_rs_half_res")}
    pad = (-c.N) % 4
    res4, res_odd = _strided(c.residual, 8 + pad), _strided(c.residual, 9 if c.N % 2 == 0 else 8)
    assert res4.stride(0) % 4 == 0 and res_odd.stride(0) % 2 == 1
    ran = set()
    for dtype in (F32, BF16):
        for kind in G.LD_KINDS:
            for epi in MATRIX_EPILOGUES:
                if epi == "inplace" and dtype != F32:
                    continue  # (the residual is float32 by contract)
                win = G.Window(c.M, c.N, dtype, kind, DEV)
                spec = epi if epi in ("none", "bias_relu") else "bias_rs_half_res"
                residual = {"res4": res4, "res_odd": res_odd}.get(epi)
                if epi == "inplace":
                    win.view.copy_(c.residual)
                    residual = win.view
                win.snapshot()
                e = _epilogue(c, spec, dtype, residual)
                expect = kernel
                if kernel == G.WS512 and not (dtype == BF16 and kind == "a8" and spec != "bias_rs_half_res"):
                    expect = TILE_KERNELS
                ran.add(_gemm(lib, c.a, c.w, win, e, expect, expect_epi1=(kernel == G.WS512 and expect == kernel)))
                msg = G.check_window(win, _want(refs[spec], dtype), tile)
                assert msg is None, "%s %s %s %s: %s" % (name, dtype, kind, epi, msg)
    assert kernel in ran
    # strided A: a column slice of a wider buffer
    wide = torch.full((c.M, 3 * c.K), 2.0, dtype=BF16, device=DEV)
    wide[:, c.K:2 * c.K] = c.a
    for dtype in (F32, BF16):
        win = G.Window(c.M, c.N, dtype, "a8", DEV).snapshot()
        _gemm(lib, wide[:, c.K:2 * c.K], c.w, win, _epilogue(c, "bias_relu", dtype), kernel if dtype == BF16 or kernel != G.WS512 else TILE_KERNELS)
        msg = G.check_window(win, _want(refs["bias_relu"], dtype), tile)
        assert msg is None, "%s %s strided A: %s" % (name, dtype, msg)


@pytest.mark.parametrize("name", list(G.KERNEL_SHAPES))
def test_addresses(lib, name):
    """One-hot rows of A: out[m, n] = W[n, hot_k(m)]; a wrong element names the (m, n, k) it came from."""
    kernel, M, N, K = G.KERNEL_SHAPES[name]
    a, w, want = [x.to(DEV) for x in G.address_case(M, N, K)]
    for dtype in (BF16,) if kernel == G.WS512 else (F32, BF16):  # (|W| <= 125: exact in bf16)
        win = G.Window(M, N, dtype, "a8", DEV).snapshot()
        e = _epilogue(None, "none", dtype)
        _gemm(lib, a, w, win, e, kernel)
        msg = G.check_window(win, want.to(dtype), G.KERNEL_TILE[kernel], explain=lambda r, col, got: G.explain_address(r, col, got, M, N, K))
        assert msg is None, "%s %s: %s" % (name, dtype, msg)


# ---- EPI = 1: column affine, second activation, sigmoid / tanh ---------------------------------------------------------------------------
def _record(got, ref, bound):
    err, live = (got.double() - ref).abs(), bound > 0  # (a zero row_scale leaves a bound of 0 and an exact 0)
    return float((err[live] / bound[live]).max()), float(err.max())


@pytest.mark.parametrize("name", list(G.KERNEL_SHAPES))
def test_epi1(lib, name):
    """bias -> ReLU -> integer column affine -> row_scale: exact.  The same with tanh behind the affine (the ECAPA chain), sigmoid,
    swish and tanh alone: float32 within the derived per-element bound, bf16 within the interval it implies.  Every shape but the
    weight-stationary ones has a column tile that crosses N."""
    kernel = G.KERNEL_SHAPES[name][0]
    tile = G.KERNEL_TILE[kernel]
    c = _case(name)
    ref, _ = G.epilogue_ref(c.z(), c, "epi1_affine")
    for dtype in (F32, BF16):
        for kind in ("a8", "a4", "odd"):
            win = G.Window(c.M, c.N, dtype, kind, DEV).snapshot()
            expect = kernel if kernel != G.WS512 or (dtype == BF16 and kind == "a8") else TILE_KERNELS
            _gemm(lib, c.a, c.w, win, _epilogue(c, "epi1_affine", dtype), expect, expect_epi1=True)
            msg = G.check_window(win, _want(ref, dtype), tile)
            assert msg is None, "%s %s %s epi1_affine: %s" % (name, dtype, kind, msg)
    ca = _case(name, act=True)
    for epi in G.NON_EXACT:
        ref, bound = G.epilogue_ref(ca.z(), ca, epi)
        y = ca.z() + ca.bias.double()
        if epi == "epi1_chain_tanh":
            y = y.clamp(min=0) * ca.col_scale.double() + ca.col_shift.double()
        assert float((y.abs() <= 4).double().mean()) >= 0.5  # the precondition, on the whole matrix
        for kind in ("a8", "odd"):
            win = G.Window(ca.M, ca.N, F32, kind, DEV).snapshot()
            # (swish is an EPI = 0 activation; the others run the EPI = 1 instantiation)
            _gemm(lib, ca.a, ca.w, win, _epilogue(ca, epi, F32), kernel if kernel != G.WS512 else TILE_KERNELS, expect_epi1=(epi != "swish"))
            ratio, worst = _record(win.view, ref, bound)
            print("%s %s %s float32: max |err| / bound %.3f, max |err| %.3e (%.2f u)" % (name, epi, kind, ratio, worst, worst / G.U))
            msg = G.check_window(win, ref, tile, bound=bound)
            assert msg is None, "%s %s %s float32: %s" % (name, epi, kind, msg)
            win = G.Window(ca.M, ca.N, BF16, kind, DEV).snapshot()
            _gemm(lib, ca.a, ca.w, win, _epilogue(ca, epi, BF16), kernel if kernel != G.WS512 or kind == "a8" else TILE_KERNELS)
            lo, hi = G.bf16_interval(ref, bound)
            msg = G.check_window(win, None, tile, lo=lo, hi=hi)
            assert msg is None, "%s %s %s bf16: %s" % (name, epi, kind, msg)
            step = G.bf16_step(ref.float().bfloat16().double())
            assert bool(((win.view.double() - ref.float().bfloat16().double()).abs() <= step + bound).all())


# ---- non-temporal stores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.NT_SHAPES))
def test_non_temporal_stores(lib, name):
    """A bf16 output of >= 2^24 elements sets nt_out without any environment switch (asserted through the query's NT flag)."""
    kernel = G.NT_SHAPES[name][0]
    c = _case(name)
    assert c.M * c.N >= 2 ** 24
    for epi in ("none", "bias_relu"):
        ref, _ = G.epilogue_ref(c.z(), c, epi)
        win = G.Window(c.M, c.N, BF16, "a8", DEV).snapshot()
        _gemm(lib, c.a, c.w, win, _epilogue(c, epi, BF16), kernel, expect_nt=True)
        msg = G.check_window(win, _want(ref, BF16), G.KERNEL_TILE[kernel])
        assert msg is None, "%s %s: %s" % (name, epi, msg)


# ---- Conv1d taps ------------------------------------------------------------------------------------------------------------------------
def _taps(lib, c, win, e, expect_kernel):
    act = c.buf[c.margin:]
    v = lib.ma_conv1d_taps_bf16_variant(c.rows, c.C, c.taps, c.dil, win.ld, c.N, ctypes.byref(e), _ptr(win.view), 0)
    assert v & 0xF == expect_kernel and v & 0x10 and (v >> 5) & 3 == 2, hex(v)
    rc = lib.ma_conv1d_taps_bf16(_ptr(act), c.buf.stride(0), c.rows, c.C, c.taps, c.dil, _ptr(c.w), _ptr(win.view), win.ld, c.N,
                                 ctypes.byref(e), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", G.TAP_SHAPES + [G.TAP_BIG], ids=lambda s: "x".join(str(v) for v in s))
def test_conv1d_taps(lib, shape):
    """out[m, n] = sum_j sum_c act[m + (j - taps / 2) dil, c] W[n, j, c] with row_scale zeroing the halo rows, and with the ECAPA
    affine (bias -> ReLU -> affine -> row_scale): exact, float32 and bf16, guard rows above and below the output window.  The
    margins of the activation buffer hold data: a tap that reads one row off changes the result."""
    c = G.TapCase(*shape, seed=3).to(DEV)
    kernel = G.T128X2 if shape == G.TAP_BIG else G.T64X3
    for epi in ("bias_rs", "epi1_affine"):
        ref, _ = G.epilogue_ref(c.z(), c, epi)
        assert bool((ref[:c.halo] == 0).all()) and bool((ref[c.rows - c.halo:] == 0).all())
        for dtype in (F32, BF16):
            for kind in ("a8", "odd"):
                win = G.Window(c.rows, c.N, dtype, kind, DEV).snapshot()
                _taps(lib, c, win, _epilogue(c, epi, dtype), kernel)
                msg = G.check_window(win, _want(ref, dtype), G.KERNEL_TILE[kernel])
                assert msg is None, "%s %s %s %s: %s" % (shape, epi, dtype, kind, msg)


# ---- Conv2d 3x3 stride 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.CONV2D_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv2d_3x3s2(lib, shape):
    c = G.Conv2dCase(*shape, seed=4).to(DEV)
    for epi in ("bias", "bias_relu"):
        ref, _ = G.epilogue_ref(c.z(), c, epi)
        for dtype in (F32, BF16):
            win = G.Window(c.M, c.N, dtype, "tight", DEV).snapshot()  # (no leading dimension: guard rows only)
            e = _epilogue(c, epi, dtype)
            rc = lib.ma_conv2d_3x3s2_nhwc_bf16(_ptr(c.act), c.B, c.H, c.Wd, c.C, _ptr(c.w), c.Cout, _ptr(win.view), ctypes.byref(e), _stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            msg = G.check_window(win, _want(ref, dtype), G.TILES["t64"])
            assert msg is None, "%s %s %s: %s" % (shape, epi, dtype, msg)


# ---- split-K ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", G.SPLITK_NS)
def test_splitk(lib, N):
    """ma_gemm_bf16_splitk_f32 at the smallest K its plan splits (read from ma_gemm_splitk_workspace_bytes): exact, with a guard band
    around the output and canary slack on both sides of the workspace."""
    M = G.SPLITK_M
    K = next(k for k in range(64, 8192, 64) if lib.ma_gemm_splitk_workspace_bytes(M, N, k) > M * N * 4)
    assert lib.ma_gemm_splitk_workspace_bytes(M, N, K - 64) == M * N * 4 if K > 64 else True
    nbytes = lib.ma_gemm_splitk_workspace_bytes(M, N, K)
    assert nbytes % (M * N * 4) == 0 and nbytes // (M * N * 4) >= 2
    c = G.Case(M, N, K, seed=6).to(DEV)
    slack = 256  # int32 elements: 1 KiB on either side
    for alpha, accumulate, kind in ((1.0, 0, "a8"), (0.5, 1, "odd"), (2.0, 1, "a4"), (2.0, 0, "odd")):
        ws = torch.full((slack + nbytes // 4 + slack,), G.F32_CANARY, dtype=torch.int32, device=DEV)
        win = G.Window(M, N, F32, kind, DEV)
        if accumulate:
            win.view.copy_(c.residual)
        win.snapshot()
        rc = lib.ma_gemm_bf16_splitk_f32(_ptr(c.a), c.a.stride(0), _ptr(c.w), c.w.stride(0), _ptr(win.view), win.ld, M, N, K, alpha,
                                         accumulate, _ptr(ws[slack:]), nbytes, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        want = alpha * c.z() + (c.residual.double() if accumulate else 0.0)
        msg = G.check_window(win, want.float(), G.TILES["t64"])
        assert msg is None, "N %d K %d alpha %s accumulate %d %s: %s" % (N, K, alpha, accumulate, kind, msg)
        assert bool((ws[:slack] == G.F32_CANARY).all()) and bool((ws[slack + nbytes // 4:] == G.F32_CANARY).all())
        assert not bool((ws[slack:slack + nbytes // 4] == G.F32_CANARY).any())  # every split wrote all of its M x N part
