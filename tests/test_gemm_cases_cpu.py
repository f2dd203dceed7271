"""CPU: the machinery of test_gemm_exact_gpu.py checked without a device.  (1) Every case's preconditions: the exactness bound, ties in
the bf16 cases, the share of small pre-activations, the halo of the tap cases, and - through the host query at 256 CUs - that every
shape selects the kernel it is meant for.  (2) The int64, float64 and torch convolution references agree.  (3) check_window rejects
each defect a kernel of csrc/gemm_bf16.hip could have, planted in the reference output; (4) the whole-tensor check of
test_conformer_ops_gpu.py accepts two of them on its own shapes.  What (4) found: a bf16 output truncated EVERYWHERE fails the old
check too (an element near the maximum errs by up to a whole step against a tolerance of half a step of the maximum); it passes when
the truncation sits in one store path only - here the per-element body of the last partial column quad."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402


# ---- (1) preconditions ---------------------------------------------------------------------------------------------------------------
ALL_PLAIN = dict(G.KERNEL_SHAPES)
ALL_PLAIN.update(G.NT_SHAPES)


@pytest.mark.parametrize("name", sorted(ALL_PLAIN))
def test_plain_case_preconditions(name):
    _, M, N, K = ALL_PLAIN[name]
    assert G.exact_bound(K) < 2 ** 23
    c = G.Case(M, N, K, seed=1)
    assert float(c.a.abs().max()) == 2 and float(c.w.abs().max()) == 2
    assert abs(float((c.a != 0).float().mean()) - 0.5) < 0.02
    assert float(c.bias.abs().max()) <= 4 * K * 1.5 / 128 and float(c.residual.abs().max()) <= 8
    assert set(c.row_scale.tolist()) == {0.0, 1.0, 2.0}
    # ties: the hot rows' outputs with the bias, before the bf16 rounding; both kinds (the even neighbour below / above)
    zh = c.a[c.hot_rows].double() @ c.w.double().T + c.bias.double()
    ties = G.is_tie(zh)
    assert int(ties.sum()) >= 2 * len(c.hot_rows)
    f = zh.float()[ties]
    assert bool((f.bfloat16().float() < f).any()) and bool((f.bfloat16().float() > f).any())
    assert bool((G.truncate_bf16(f) != f.bfloat16()).any())
    assert M - 1 in c.hot_rows
    if name in G.KERNEL_SHAPES:  # a ragged last row tile and, but for the weight-stationary kernel, a ragged last column tile
        assert M % 256 != 0 and M % 32 != 0 and (ALL_PLAIN[name][0] == G.WS512 or N % 128 != 0)
        assert ALL_PLAIN[name][0] == G.WS512 or N % 4 != 0 or name == "8ph_row"  # (1700: the blocked-order shape brings N % 4 == 2)
    # the activation case of the same shape
    ca = G.Case(M, N, K, density=G.act_density(K), seed=2, hot=False)
    for epi in G.NON_EXACT:
        assert G.small_z_share(ca, epi) >= 0.5, epi


@pytest.mark.parametrize("shape", G.TAP_SHAPES + [G.TAP_BIG])
def test_tap_case_preconditions(shape):
    rows, C, taps, dil, N = shape
    assert G.exact_bound(C, taps) < 2 ** 23
    c = G.TapCase(rows, C, taps, dil, N, seed=3)
    assert c.margin >= (taps // 2) * dil and c.buf.shape[0] == rows + 2 * c.margin
    assert float(c.buf[:c.margin].abs().max()) == 2 and float(c.buf[-c.margin:].abs().max()) == 2  # margins hold data, not zeros
    assert bool((c.row_scale[:c.halo] == 0).all()) and bool((c.row_scale[rows - c.halo:] == 0).all())
    assert bool((c.row_scale[c.halo:rows - c.halo] > 0).all())
    if rows <= 200:
        z = c.z_int64()
        assert bool((z.double() == c.z()).all()) and bool((c.z_conv1d() == c.z()).all())
        inner = [r for r in G.hot_indices(rows) if c.row_scale[r] > 0]
        assert inner and int(G.is_tie((c.z()[inner] + c.bias.double()).float()).sum()) >= 2


@pytest.mark.parametrize("shape", G.CONV2D_SHAPES)
def test_conv2d_case_references_agree(shape):
    c = G.Conv2dCase(*shape, seed=4)
    assert G.exact_bound(c.K) < 2 ** 23
    z = c.columns().long() @ c.w.reshape(c.Cout, -1).long().T
    assert bool((z.double() == c.z()).all()) and bool((c.z_conv2d() == c.z()).all())
    assert int(G.is_tie((c.z()[:1] + c.bias.double()).float()).sum()) >= 2


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _build, _lib

    _build.build()
    return _lib.load()


def _variant(lib, M, N, K, ldo, out=4096, cus=256, **fields):
    from mindaudio_amd import _lib

    e = _lib.GemmEpilogue()
    e.alpha = 1.0
    for k, v in fields.items():
        setattr(e, k, v)
    return lib.ma_gemm_bf16_variant(M, N, K, ldo, ctypes.byref(e), out, cus)


@pytest.mark.parametrize("name", sorted(ALL_PLAIN))
def test_shapes_select_their_kernel_at_256_cus(lib, name):
    kernel, M, N, K = ALL_PLAIN[name]
    ld = G.ld_off(N, "a8")[0]
    for bf16 in ((1,) if kernel == G.WS512 else (0, 1)):
        v = _variant(lib, M, N, K, ld, out_bf16=bf16)
        assert v & 0xF == kernel, (name, hex(v))
        assert bool(v & 0x100) == bool(bf16 and M * N >= 2 ** 24)
        v = _variant(lib, M, N, K, ld, out_bf16=bf16, act=G.ACT_SIGMOID)
        assert v & 0xF == kernel and v & 0x10
    if kernel == G.WS512:  # what its dispatch condition rejects falls to a tile kernel
        for kw in (dict(out_bf16=0), dict(out_bf16=1, residual=4096, ldr=N), dict(out_bf16=1, alpha=0.5), dict(out_bf16=1, out=4096 + 8)):
            out = kw.pop("out", 4096)
            assert _variant(lib, M, N, K, ld, out=out, **kw) & 0xF in (G.T128X2, G.T64X2, G.T64X3), kw
        assert _variant(lib, M, N, K, G.ld_off(N, "a4")[0], out_bf16=1) & 0xF != G.WS512


def test_variant_query_refuses_what_the_launch_refuses(lib):
    from mindaudio_amd import _lib

    assert _variant(lib, 131, 301, 100, 304) == -5   # K % 64
    assert _variant(lib, 131, 301, 128, 300) == -5   # ldo < N
    assert _variant(lib, 131, 301, 128, 304, act=5) == -1
    assert _variant(lib, 131, 301, 128, 304, residual=4096, ldr=300) == -1
    assert _variant(lib, 131, 301, 128, 304, out=0) == -1
    assert lib.ma_gemm_bf16_variant(131, 301, 128, 304, None, 4096, 256) == G.T64X3
    e = _lib.GemmEpilogue()
    e.alpha = 1.0
    rows, C, taps, dil, N = G.TAP_BIG
    v = lib.ma_conv1d_taps_bf16_variant(rows, C, taps, dil, G.ld_off(N, "a8")[0], N, ctypes.byref(e), 4096, 256)
    assert v & 0xF == G.T128X2 and v & 0x10 and (v >> 5) & 3 == 2
    for rows, C, taps, dil, N in G.TAP_SHAPES:
        v = lib.ma_conv1d_taps_bf16_variant(rows, C, taps, dil, G.ld_off(N, "a8")[0], N, ctypes.byref(e), 4096, 256)
        assert v & 0xF == G.T64X3 and (v >> 5) & 3 == 2
    assert lib.ma_conv1d_taps_bf16_variant(200, 64, 2, 1, 128, 100, ctypes.byref(e), 4096, 256) == -1  # even tap count
    assert lib.ma_conv1d_taps_bf16_variant(200, 64, 1, 1, 128, 100, ctypes.byref(e), 4096, 256) == (G.T64X3 | 0x10)


# ---- (2) references ------------------------------------------------------------------------------------------------------------------
def test_int64_and_float64_references_agree():
    c = G.Case(131, 301, 128, seed=1)
    assert bool((G.z_int64(c.a, c.w).double() == c.z()).all())
    z = G.z_int64(c.a, c.w)
    for name in ("none", "bias_relu", "bias_rs_half_res", "epi1_affine"):
        ref, bound = G.epilogue_ref(c.z(), c, name)
        assert bound is None
        e = G.EPILOGUES[name]
        v = z + c.bias.long() if e.get("bias") else z.clone()
        if e.get("act") == G.ACT_RELU:
            v = v.clamp(min=0)
        if e.get("affine"):
            v = v * c.col_scale.long() + c.col_shift.long()
        v2 = v * (c.row_scale.long()[:, None] if e.get("row_scale") else 1)  # twice the value where alpha = 0.5
        two_ref = v2 if e.get("alpha") == 0.5 else 2 * v2
        if e.get("residual"):
            two_ref = two_ref + 2 * c.residual.long()
        assert bool((two_ref.double() == 2 * ref).all()), name
        assert bool((ref.float().double() == ref).all())  # exact in float32
        assert float(ref.abs().max()) <= G.exact_bound(c.K)


def test_address_case_names_its_source():
    a, w, want = G.address_case(131, 301, 128)
    assert bool(((a.double() @ w.double().T).float() == want).all())
    assert bool((a.sum(1) == 1).all()) and float(w.abs().max()) <= 125
    msg = G.explain_address(5, 7, float(want[5, 8]), 131, 301, 128)
    assert "n in [" in msg and "8" in msg.split("n in ")[1].split("]")[0]


def test_activation_bounds_hold_for_a_float32_model_and_are_tight():
    """act_bound against a float32 evaluation of apply_act's formulas with correctly rounded exp2 / reciprocal (a stand-in for the
    instructions: at most half of their stated error), and against a float32 value pushed off by 4 ulp (rejected where the value is
    not tiny)."""
    y = torch.arange(-120, 121, dtype=torch.float64)
    for act, c in ((G.ACT_SIGMOID, -1.4426950408889634), (G.ACT_SWISH, -1.4426950408889634), (G.ACT_TANH, -2.8853900817779268)):
        yf = y.float()
        r = (1.0 / (1.0 + torch.exp2(torch.tensor(c, dtype=torch.float32) * yf)))
        got = r if act == G.ACT_SIGMOID else yf * r if act == G.ACT_SWISH else 2.0 * r - 1.0
        ref, bound = G.act64(y, act), G.act_bound(y, act)
        assert bool(((got.double() - ref).abs() <= bound).all()), act
        mid = (y.abs() <= 4) & (y != 0)
        assert bool(((ref * (1 + 2.0 ** -19))[mid].sub(ref[mid]).abs() > bound[mid]).all()), act  # 32 ulp off is outside
    assert float(G.act_bound(torch.zeros(1, dtype=torch.float64), G.ACT_TANH)) <= 6 * G.U  # the absolute term at the cancellation


# ---- (3) planted defects -------------------------------------------------------------------------------------------------------------
def _window_with(want, kind="a8", inplace_residual=None):
    win = G.Window(want.shape[0], want.shape[1], want.dtype, kind)
    if inplace_residual is not None:
        win.view.copy_(inplace_residual)
    win.snapshot()
    win.view.copy_(want)
    return win


@pytest.fixture(scope="module")
def small():
    c = G.Case(131, 301, 128, seed=1)
    return c, c.z()


def test_comparator_accepts_the_reference(small):
    c, z = small
    for name in ("none", "bias_relu", "bias_rs_half_res", "epi1_affine"):
        ref, _ = G.epilogue_ref(z, c, name)
        for want in (ref.float(), ref.float().bfloat16()):
            for kind in G.LD_KINDS:
                assert G.check_window(_window_with(want, kind), want) is None


def test_defect_partial_quad_takes_left_bias(small):
    c, z = small
    ref, _ = G.epilogue_ref(z, c, "bias_relu")
    want = ref.float()
    q = c.N - c.N % 4
    shifted = c.bias.clone()
    shifted[q:] = c.bias[q - 1:c.N - 1]
    got = (z + shifted.double()).clamp(min=0).float()
    assert bool((got[:, :q] == want[:, :q]).all())
    msg = G.check_window(_window_with(got), want)
    assert msg and any("column %d)" % n in msg for n in range(q, c.N))


def test_defect_last_row_written_into_the_guard_row(small):
    c, z = small
    want = G.epilogue_ref(z, c, "bias_relu")[0].float()
    win = _window_with(want)
    win.buf[win.top + c.M, win.off:win.off + c.N] = want[c.M - 1]
    msg = G.check_window(win, want)
    assert msg and "guard band" in msg and "window row %d of %d" % (c.M, c.M) in msg
    assert G.old_check_f32(win.view, want)  # the old check looks at the (M, N) window only


def test_defect_guard_columns_and_top_rows():
    want = torch.ones(5, 9)
    for r, col in ((0, 0), (1, 30), (3, 7), (4, 17), (9, 10)):
        win = _window_with(want)
        win.buf[r, col] = 1.0
        assert "guard band" in G.check_window(win, want)


def test_defect_one_k_tile_dropped_from_one_tile(small):
    c, z = small
    want = z.float()
    a2 = c.a.clone()
    a2[:, 64:128] = 0
    got = want.clone()
    got[64:128, 128:256] = (a2.double() @ c.w.double().T).float()[64:128, 128:256]
    msg = G.check_window(_window_with(got), want, tile=G.TILES["t64"])
    assert msg and "tile (1, 1)" in msg


def test_defect_one_tap_reads_one_row_off():
    c = G.TapCase(200, 64, 3, 2, 100, seed=3, extra_margin=1)
    want = c.z().float()
    for j in range(3):
        got = c.z_int64(off_by_one_tap=j).float()
        assert G.check_window(_window_with(got), want) is not None


def test_defect_bf16_truncated(small):
    c, z = small
    ref = G.epilogue_ref(z, c, "bias_relu")[0].float()
    want, got = ref.bfloat16(), G.truncate_bf16(ref)
    msg = G.check_window(_window_with(got), want)
    assert msg and "wrong elements" in msg
    # round-half-up (away from zero) differs from nearest-even at the planted ties only
    up = torch.where(G.is_tie(ref) & (want.float().abs() < ref.abs()), (ref * (1 + 2.0 ** -9)).bfloat16(), want)
    assert int((up != want).sum()) >= 1 and G.check_window(_window_with(up), want) is not None


def test_defect_residual_added_twice_in_place(small):
    c, z = small
    want = G.epilogue_ref(z, c, "bias_rs_half_res")[0].float()
    got = (want.double() + c.residual.double()).float()
    assert G.check_window(_window_with(got, inplace_residual=c.residual), want) is not None


def test_defect_row_scale_of_the_clamped_row(small):
    c, z = small
    want = G.epilogue_ref(z, c, "epi1_affine")[0].float()
    c2 = G.Case(131, 301, 128, seed=1)
    c2.row_scale[128:] = c2.row_scale[c.M - 1]  # the rows of the last tile read row_scale[M - 1]
    assert bool((c2.row_scale != c.row_scale).any()), "the case must hold different scales in its last tile"
    got = G.epilogue_ref(z, c2, "epi1_affine")[0].float()
    msg = G.check_window(_window_with(got), want, tile=G.TILES["t64"])
    assert msg and "tile (2," in msg


def test_defect_8ph_tile_order_is_no_bijection():
    c = G.Case(600, 700, 64, seed=5)
    want = c.z().float()
    tiles_n, ntiles = 3, 9
    perm = G.tile_permutation_defect(ntiles, twice=2, never=7)
    assert sorted(set(perm)) != list(range(ntiles))
    win = G.Window(c.M, c.N, torch.float32).snapshot()
    for tile in perm:  # every workgroup writes the tile it was given
        r0, c0 = tile // tiles_n * 256, tile % tiles_n * 256
        win.view[r0:r0 + 256, c0:c0 + 256] = want[r0:r0 + 256, c0:c0 + 256]
    msg = G.check_window(win, want, tile=G.TILES["8ph"])
    assert msg and "tile (2, 1)" in msg and "position (0, 0)" in msg


# ---- (4) what the whole-tensor check of test_conformer_ops_gpu.py does not see ----------------------------------------------------------
def test_old_check_accepts_truncation_in_the_partial_quad_on_its_own_shape():
    m, n, k = 333, 4233, 256  # of test_gemm_plain_and_transpose_detecting, with its inputs

    def rand(*shape, seed, scale=1.0):
        return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale

    a, w, bias = rand(m, k, seed=1).bfloat16(), rand(n, k, seed=2, scale=1.0 / math.sqrt(k)).bfloat16(), rand(n, seed=3)
    ref = a.double() @ w.double().T + bias.double()
    want = ref.float().bfloat16()
    got = want.clone()
    q = n - n % 4
    got[:, q:] = G.truncate_bf16(ref.float()[:, q:])
    assert int((got != want).sum()) > 100
    assert G.old_check_bf16(got, ref)                                   # accepted
    assert G.check_window(_window_with(got), want) is not None          # rejected
    assert not G.old_check_bf16(G.truncate_bf16(ref.float()), ref)      # (truncated everywhere, the old check fails too)
