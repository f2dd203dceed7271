"""CPU: the cases of packed_cases.py meet the conditions their exactness rests on, the comparators used by test_packed_exact_gpu.py
reject every planted defect, and the whole-tensor tolerances of test_conformer_ops_gpu.py accept the first group of them (the gap
the exact tests close)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402
import packed_cases as P  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16


def _x_window(M, values, kind="a4"):
    win = G.Window(M, 256, F32, kind)
    win.snapshot()
    win.view.copy_(values)
    return win


# ---- FFN: conditions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln_in", [False, True])
@pytest.mark.parametrize("hidden", P.FFN_HIDDENS)
def test_saturated_case_conditions(hidden, ln_in):
    c = P.FfnCase(193, hidden, "sat", ln_in=ln_in, seed=1, alpha=0.5)
    y = c.y()
    assert bool((y == y.round()).all()) and 16 <= float(y.min()) and float(y.max()) <= 255
    # every row of W1: one non-zero per k-step, and over the units every k mod 32 is used
    nz = (c.w1.float() != 0).view(hidden, 8, 32)
    assert bool((nz.sum(-1) == 1).all()) and bool(nz.any(0).all())
    # bf16(swish(y)) == y with the kernels' float32 chain, also with the reciprocal 4 ULP off either way
    for ulps in (0, -4, 4):
        assert torch.equal(P.swish_chain32(y, ulps).bfloat16().double(), y)
    assert torch.equal(G.act64(y, G.ACT_SWISH).float().bfloat16().double(), y)
    # all partial sums of the second product, the bias, alpha and the residual stay below 2^23 in units of 1/2
    worst = float((y.abs() @ c.w2.double().abs().T).max()) + 3 + 8
    assert 2 * worst < 2 ** 23
    x = c.x_ref()
    assert bool((2 * x == (2 * x).round()).all()) and torch.equal(x.float().double(), x)
    # ... and the int64 evaluation agrees with the float64 one
    o = y.long() @ c.w2.long().T + c.b2.long()
    assert torch.equal(c.x0.double() + 0.5 * o.double(), x)


@pytest.mark.parametrize("ln_in", [False, True])
def test_interval_case_conditions(ln_in):
    c = P.FfnCase(193, 512, "act", ln_in=ln_in, seed=2)
    y = c.y()
    assert bool((y == y.round()).all()) and float(y.abs().max()) < 2 ** 23
    if not ln_in:
        assert float((y.abs() <= 4).double().mean()) >= 0.5
    assert sorted(P.PI.tolist()) == list(range(256))
    for p in range(c.passes()):
        lo, hi = c.x_ref(p)
        yp = y[:, 256 * p + P.PI]
        single = (lo == hi) | (yp == 0)   # one bf16 number everywhere but at y = 0 (where it is [-tiny, +tiny])
        assert bool(single.all())
        h = P.swish_chain32(yp).bfloat16().float()
        assert bool(((c.x0 + h >= lo) & (c.x0 + h <= hi)).all())
        # truncation and a missing bias leave the interval
        ht = G.truncate_bf16(P.swish_chain32(yp)).float()
        assert float((~((c.x0 + ht >= lo) & (c.x0 + ht <= hi))).float().mean()) > 0.2
        y0 = (y - c.b1.double())[:, 256 * p + P.PI]
        h0 = P.swish_chain32(y0).bfloat16().float()
        bad = ~((c.x0 + h0 >= lo) & (c.x0 + h0 <= hi))
        live = (c.b1[256 * p + P.PI] != 0)[None, :] & (yp != 0) & (y0 != yp)
        if ln_in:  # (x0 = +-s absorbs the Swish values far below its own last bit: y << 0 with or without the bias)
            assert float(bad[live.expand_as(bad)].float().mean()) > 0.5
        else:
            assert bool(bad[live.expand_as(bad)].all())


def test_input_layernorm_identity():
    """bf16(LN(x0) gamma0 + beta0) == sign * gamma0 + beta0 under three float32 formulas / summation orders."""
    x0, sign = P.balanced_rows(193, 5)
    g0, b0 = P.ln_params_exact(9)
    want = (sign * g0 + b0).bfloat16()
    assert bool((want.float() != 0).all()) and torch.equal(want.float(), sign * g0 + b0)
    assert torch.equal(P.ln32_two_pass(x0, g0, b0, 1e-5).bfloat16(), want)
    assert torch.equal(P.ln32(x0, g0, b0, 1e-5, "lanes").bfloat16(), want)
    assert torch.equal(torch.nn.functional.layer_norm(x0, (256,), g0, b0, 1e-5).bfloat16(), want)
    # a beta that cancels gamma breaks it (why |beta0| >= 3): the exact zeros come out as +-tiny
    bz = torch.full((256,), -1.0)
    assert not torch.equal(P.ln32_two_pass(x0, torch.ones(256), bz, 1e-5).bfloat16(), (sign - 1).bfloat16())


# ---- LayerNorm bound -----------------------------------------------------------------------------------------------------------------
def _ln_inputs():
    """Stage inputs as the GPU test meets them: the exact x of a saturated case (variance ~ 1e6), and a first-stage output."""
    c = P.FfnCase(65, 256, "sat", seed=3, alpha=0.5)
    x = c.x_ref().float()
    g1 = P._choice((-128.0, -64.0, -32.0, 32.0, 64.0, 128.0), 256, 31)
    be1 = G.int_vector(256, -3, 3, 32)
    g2, be2 = P.ln_params_exact(33)
    return x, (g1, be1), (g2, be2)


LN_EPS = 4096.0


def test_layernorm_bound_holds_and_rejects():
    x, (g1, be1), (g2, be2) = _ln_inputs()
    x1 = P.ln32(x, g1, be1, LN_EPS, "lanes")
    for v, (ga, be), (go, bo) in ((x, (g1, be1), (g2, be2)), (x1, (g2, be2), (g1, be1))):
        ref, bound = P.ln_bound(v, ga, be, LN_EPS)
        worst = 0.0
        for order in ("lanes", "tree", "k256"):
            got = P.ln32(v, ga, be, LN_EPS, order).double()
            assert bool(((got - ref).abs() <= bound).all()), order
            worst = max(worst, float(((got - ref).abs() / bound).max()))
            lo, hi = G.bf16_interval(ref, bound)
            gb = got.float().bfloat16()
            assert bool(((gb.double() >= lo.double()) & (gb.double() <= hi.double())).all())
        assert worst > 0.002, worst  # the bound is not vacuous: float32 arithmetic comes within a factor of 500 of it
        # the bound is tight against the stage's scale: at most 1e-5 of the largest output
        assert float(bound.max()) <= 1e-5 * float(ref.abs().max())
        for name, bad in (("no eps", P.ln32(v, ga, be, LN_EPS, use_eps=False)), ("N - 1", P.ln32(v, ga, be, LN_EPS, ddof=1)),
                          ("other stage's gamma / beta", P.ln32(v, go, bo, LN_EPS))):
            win = _x_window(65, bad)
            msg = G.check_window(win, ref, P.FFN_TILE, bound=bound)
            assert msg is not None and "tile (0, 0)" in msg, name
    # a zero row scale leaves an exact zero and a zero bound
    rs = torch.tensor([0.0, 1.0] * 32 + [1.0])
    ref, bound = P.ln_bound(x, g2, be2, 1e-5, row_scale=rs)
    assert bool((ref[0] == 0).all()) and bool((bound[0] == 0).all()) and bool((bound[1] > 0).all())


# ---- qkv tail ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", P.QKV_NS)
def test_qkv_case_ties(N):
    c = P.QkvCase(193, N, seed=4)
    assert torch.equal(P.ln32(c.x0, c.gamma1, c.beta1, 1e-5, "lanes").bfloat16().float(), c.a1)
    ref = c.ref()
    assert float(ref.abs().max()) < 2 ** 23 and torch.equal(ref.float().double(), ref)
    share, even, odd = P.tie_stats(ref)
    assert share >= 0.01 and even > 0 and odd > 0, (share, even, odd)
    want = ref.float().bfloat16()
    # truncation and round-half-up are both rejected
    assert not torch.equal(G.truncate_bf16(ref.float()), want)
    up = ((ref.float().view(torch.int32) + 0x8000) & -65536).view(F32).bfloat16()
    assert not torch.equal(up, want)


# ---- planted defects -----------------------------------------------------------------------------------------------------------------
# (the units are positions: hidden units on the random case, output columns of the interval case)
FIRST_GROUP = (("trunc_h", ()), ("no_b1", range(8)), ("drop_last_kstep", range(32, 36)), ("exp_const", ()))
OLD_TOL_250_2048 = 0.043  # 3e-3 max |xs| of test_ffn_packed's (250, 2048) case: the restated operands are the test's own


def test_old_tolerances_accept_the_first_group():
    o = P.old_ffn_case()
    args = (o["a"], o["w1"], o["b1"], o["w2"], o["b2"], o["x0"], o["alpha"])
    xs = P.ffn_model(*args)
    for defect, units in FIRST_GROUP:
        x = P.ffn_model(*args, defect=defect, units=units)
        assert float((x - xs).abs().max()) > 0
        assert P.old_ffn_check(x, xs, o["g1"], o["be1"]) == (True, True), defect
    assert abs(OLD_TOL_250_2048 - P.OLD_FFN_X_TOL * float(xs.abs().max())) < 1e-3


@pytest.mark.parametrize("ln_in", [False, True])
def test_exact_comparators_reject_every_defect(ln_in):
    M, hidden = 193, 512
    sat = P.FfnCase(M, hidden, "sat", ln_in=ln_in, seed=1, alpha=0.5)
    want = sat.x_ref().float()
    good = _x_window(M, want)
    assert G.check_window(good, want, P.FFN_TILE) is None
    args = (sat.a, sat.w1, sat.b1, sat.w2, sat.b2, sat.x0, sat.alpha)
    for defect, units in (("no_b1", range(8)), ("drop_last_kstep", range(4)), ("drop_unit", (37,)), ("swap_b1", ()),
                          ("drop_o_block", (64,)), ("b2_unscaled", ()), ("tile_twice", ())):
        msg = G.check_window(_x_window(M, P.ffn_model(*args, defect=defect, units=units).float()), want, P.FFN_TILE)
        assert msg is not None, defect
        if defect == "tile_twice":
            assert "tile (1, 0)" in msg
    # the saturated case cannot see a truncated h or a wrong exp constant (h is an integer either way); the interval case does
    act = P.FfnCase(M, hidden, "act", ln_in=ln_in, seed=2)
    for p in range(act.passes()):
        lo, hi = act.x_ref(p)
        w2 = act.w2_pass(p)
        aargs = (act.a, act.w1, act.b1, w2, act.b2, act.x0, 1.0)
        assert G.check_window(_x_window(M, P.ffn_model(*aargs).float()), None, P.FFN_TILE, lo=lo, hi=hi) is None
        # (the k-step defect on every column: with the sparse W1 of the LayerNorm variant few units have a weight in the last k-step)
        for defect, units in FIRST_GROUP[:2] + (("drop_last_kstep", range(256)),) + FIRST_GROUP[3:]:
            u = [256 * p + int(P.PI[n]) for n in units]
            msg = G.check_window(_x_window(M, P.ffn_model(*aargs, defect=defect, units=u).float()), None, P.FFN_TILE, lo=lo, hi=hi,
                                 explain=act.explain(p))
            assert msg is not None and "hidden unit" in msg and "wave" in msg, (defect, p)
    # a 64-row tile never written, and a row written past M
    win = G.Window(M, 256, F32, "a4").snapshot()
    win.view.copy_(want)
    G._bits(win.view[64:128]).fill_(G.F32_CANARY)
    assert "tile (1, 0)" in G.check_window(win, want, P.FFN_TILE)
    win = _x_window(M, want)
    win.buf[win.top + M, win.off:win.off + 256] = 1.0
    assert "guard band" in G.check_window(win, want, P.FFN_TILE)
    win = _x_window(M, want)
    win.buf[win.top + 5, win.off + 256] = 1.0   # a column past the row's 256
    assert "guard band" in G.check_window(win, want, P.FFN_TILE)


# ---- gemm_k256 / rows_packed ---------------------------------------------------------------------------------------------------------
def test_dense_cases_conditions():
    for K in (256,) + P.ROWS_KS:
        assert 16 * G.exact_bound(K) < 2 ** 23  # (alpha 16 of rows_packed)
    for M, N in ((130, 512), (1, 256), (257, 1024)):
        c = P.DenseCase(M, N, 256, seed=11)
        for epi in ("bias", "bias_relu", "bias_rs_half_res"):
            ref, _ = G.epilogue_ref(c.z(), c, epi)
            assert bool((32 * ref == (32 * ref).round()).all()) and 32 * float(ref.abs().max()) < 2 ** 23
            share, even, odd = P.tie_stats(ref)
            if epi != "bias_rs_half_res":  # (a row scale of 0 or 2 and alpha 0.5 move the ties; M = 1 may have none)
                assert share >= 0.01 and even > 0 and odd > 0, (M, N, epi, share, even, odd)
    a, w, want = G.address_case(65, 256, 448)
    assert torch.equal(a.double() @ w.double().T, want.double())
    bad = want.clone()
    bad[3, 17] = G.address_w(17, G.hot_k(3, 448) + 8)
    win = G.Window(65, 256, F32, "a4").snapshot()
    win.view.copy_(bad)
    msg = G.check_window(win, want, P.ROWS_TILE, explain=P.explain_fragment(65, 256, 448))
    assert "k-step" in msg and "lane group" in msg


# ---- front end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmvn", [False, True])
def test_front_case_conditions(cmvn):
    c = P.FrontCase(3, 59, cmvn=cmvn, seed=6)
    a1 = c.act1()
    assert float(a1.max()) < 128 and torch.equal(a1.float().bfloat16().double(), a1)
    z = c.z2()
    assert bool((2 * z == (2 * z).round()).all())
    worst = float((c.columns().abs() @ c.w2.reshape(256, -1).double().abs().T).max()) + 3
    assert 2 * worst < 2 ** 23
    assert c.T2 * c.F2 == 266 and P.FrontCase(1, 31).T2 * 19 == 133 and P.FrontCase(1, 19).T1 == 9 and P.FrontCase(1, 7).T2 == 1
    share, even, odd = P.tie_stats(c.out())
    assert share >= 0.01 and even > 0 and odd > 0, (share, even, odd)
    want = c.out().float().bfloat16()
    assert torch.equal(torch.nn.functional.conv2d(a1.permute(0, 3, 1, 2), c.w2.double().permute(0, 3, 1, 2), c.b2.double(), stride=2)
                       .permute(0, 2, 3, 1).reshape(-1, 256), c.z2())
    # a tap read one patch position off at the first position of the second tile
    bad = c.out(seam_defect=(128, 4)).float().bfloat16()
    win = G.Window(want.shape[0], 256, BF16, "tight").snapshot()
    win.view.copy_(bad)
    msg = G.check_window(win, want, P.CONV_TILE)
    assert msg is not None and "tile (1, 0), position (0," in msg


def test_split_case_conditions():
    c = P.SplitCase(2, 41, seed=7)
    for v, h, l in ((c.x, c.xh, c.xl), (c.w1, c.wh, c.wl)):
        assert torch.equal(v.bfloat16().float(), h) and torch.equal(v - h, l) and torch.equal(l.bfloat16().float(), l)
    z = c._conv(c.xh, c.wh) + c._conv(c.xh, c.wl) + c._conv(c.xl, c.wh)
    assert float(z.abs().max()) < 64 and bool((1024 * z == (1024 * z).round()).all())
    a = c.act1()
    cancelled = (c._conv(c.xh, c.wh) + c.b1.double() == 0)
    assert float(cancelled.double().mean()) > 0.01 and float((a[cancelled] != 0).double().mean()) > 0.2  # the tails alone, where positive
    full = (c._conv(c.x, c.w1) + c.b1.double()).clamp(min=0).float().bfloat16().double()
    assert not torch.equal(full, a)  # the xl wl term is visible too: the reference must leave it out
    for p in (0, 4, 8):
        want = c.out_pass(p).float().bfloat16()
        for drop in ("xh_wl", "xl_wh"):
            win = G.Window(want.shape[0], 256, BF16, "tight").snapshot()
            win.view.copy_(c.out_pass(p, drop).float().bfloat16())
            msg = G.check_window(win, want, P.CONV_TILE, explain=c.explain_pass(p))
            assert msg is not None and "tap %d" % p in msg and "chunk" in msg, (p, drop)
        # the one-hot W2 gathers: the dense conv2 on it gives the same
        cols = c.columns().double() @ c.w2_pass(p).reshape(256, -1).double().T
        assert torch.equal(cols, c.out_pass(p))
