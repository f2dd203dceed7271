"""CPU self-test of tests/train_kernel_cases.py: the float64 references against torch float64 autograd of the plainly written
operations (1e-10 relative), and for every case the GPU test runs: a float32 restatement passes the case's check_* (the bounds are not
void for a correct implementation) and every applicable planted defect fails it (they are not so wide that a wrong one passes)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_kernel_cases as T  # noqa: E402


def close(got, want, tol=1e-10):
    return float((got.double() - want.double()).abs().max()) <= tol * max(float(want.double().abs().max()), 1e-300)


# ---- the mask ----------------------------------------------------------------------------------------------------------------------
def test_drop_params_restates_make_drop():
    assert T.drop_params(0.0) == (0, np.float32(1.0)) and T.drop_params(-1.0)[0] == 0
    th, ik = T.drop_params(0.5)
    assert th == 1 << 31 and ik == np.float32(2.0)
    th, ik = T.drop_params(0.1)  # p is the float32 0.1 = 0.100000001490116...
    assert th == int(float(np.float32(0.1)) * 2.0 ** 32) and ik == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    assert T.drop_params(1.0)[0] == 0xFFFFFFFF  # saturated (the launchers refuse p >= 1 before it gets there)
    th, ik = T.drop_params(T.P_TINY)
    assert th != 0 and th >> 16 == 0 and ik > 1  # nothing dropped, everything scaled
    assert T.real_drop_probability(0.1) == math.floor(float(np.float32(0.1)) * 65536) / 65536
    assert bool(T.keep_mask(1, 2, np.arange(4096), T.P_TINY).all())


@pytest.mark.parametrize("p", T.DROP_PS)
def test_keep_fraction(p):
    n = 1 << 20
    q = T.real_drop_probability(p)
    kept = T.keep_mask(77, 5, np.arange(n, dtype=np.uint64), p).mean()
    assert abs(kept - (1 - q)) <= 4 * math.sqrt(q * (1 - q) / n), (kept, q)


def test_one_hash_per_quad():
    """Elements 4 q .. 4 q + 3 read the 16-bit fields of ONE hash pair: low / high half of word 0, low / high half of word 1."""
    q = np.arange(5000, dtype=np.uint64) * np.uint64(977)
    x, y = T.quad_hash(9, 3, q)
    for p in T.DROP_PS:
        t = T.drop_params(p)[0] >> 16
        fields = (x & np.uint64(0xFFFF), x >> np.uint64(16), y & np.uint64(0xFFFF), y >> np.uint64(16))
        for e, f in enumerate(fields):
            assert np.array_equal(T.keep_mask(9, 3, q * np.uint64(4) + np.uint64(e), p), f >= np.uint64(t))
    # the swapped-pair defect is a different mask
    idx = np.arange(1 << 16, dtype=np.uint64)
    assert (T.keep_mask(9, 3, idx, 0.5) != T.keep_mask(9, 3, idx, 0.5, defect="mask_pair_swapped")).mean() > 0.4


def test_seed_salt_and_high_word():
    idx = np.arange(1 << 16, dtype=np.uint64)
    base = T.keep_mask(77, 5, idx, 0.5)
    for seed, salt in ((78, 5), (77, 6), (77 + (1 << 31), 5)):
        assert 0.45 < (T.keep_mask(seed, salt, idx, 0.5) != base).mean() < 0.55
    # indices at and above 2^34 (quad index >= 2^32): the high word is folded in.  No kernel test reaches such an index (a tensor of
    # 2^34 elements), so the fold is checked on this restatement only.
    high = idx + np.uint64(1 << 34)
    assert 0.45 < (T.keep_mask(77, 5, high, 0.5) != base).mean() < 0.55
    assert 0.45 < (T.keep_mask(77, 5, idx + np.uint64(1 << 35), 0.5) != T.keep_mask(77, 5, high, 0.5)).mean() < 0.55
    x0, _ = T.quad_hash(77, 5, np.array([5], dtype=np.uint64))
    x1, _ = T.quad_hash(77, 5, np.array([5 + (3 << 32)], dtype=np.uint64))
    assert int(x0[0]) != int(x1[0])


# ---- references against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.LN_WIDTHS)
def test_ln_bwd_ref_is_autograd(D):
    g = torch.Generator().manual_seed(D)
    rows = 7
    x = (torch.randn(rows, D, generator=g, dtype=torch.float64) * 2 + 0.3).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)).requires_grad_()
    beta = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    rs = torch.tensor([0.0, 1, 0.5, 1, 1, 0, 1], dtype=torch.float64)
    dy = torch.randn(rows, D, generator=g, dtype=torch.float64)
    y = F.layer_norm(x, (D,), gamma, beta, T.f32(T.EPS_LN)) * rs[:, None]
    y.backward(dy)
    g0 = torch.randn(rows, D, generator=g, dtype=torch.float64)
    got, dg, db, _ = T.ln_bwd_ref(x.detach(), gamma.detach(), dy, g0, rs, True)
    assert close(got - g0, x.grad) and close(dg, gamma.grad) and close(db, beta.grad)
    got, _, _, _ = T.ln_bwd_ref(x.detach(), gamma.detach(), dy, g0, rs, False)
    assert close(got, x.grad)


@pytest.mark.parametrize("act", (T.ACT_SWISH, T.ACT_RELU))
def test_act_refs_are_autograd(act):
    g = torch.Generator().manual_seed(act)
    u = torch.randn(1000, generator=g, dtype=torch.float64).requires_grad_()
    keep = torch.from_numpy(T.keep_mask(3, 4, np.arange(1000), 0.1)).double()
    ik = float(T.drop_params(0.1)[1])
    h = (F.silu(u) if act == T.ACT_SWISH else F.relu(u)) * keep * ik
    assert close(T.act_fwd_ref(u.detach(), act) * keep * ik, h.detach())
    dh = torch.randn(1000, generator=g, dtype=torch.float64)
    h.backward(dh)
    assert close(dh * T.act_grad_ref(u.detach(), act) * keep * ik, u.grad)


def test_subsample_refs_are_conv_autograd():
    """im2col_t_ref is the operand of the 3x3 stride-2 valid convolution; col2im_relu_ref (without its gate) its adjoint."""
    g = torch.Generator().manual_seed(5)
    b, h, w, c, co = 2, 8, 7, 5, 3
    ho, wo = T.out_hw(h, w)
    act = torch.randn(b, h, w, c, generator=g, dtype=torch.float64).requires_grad_()
    wgt = torch.randn(co, c, 3, 3, generator=g, dtype=torch.float64)
    out = F.conv2d(act.permute(0, 3, 1, 2), wgt, stride=2)  # (b, co, ho, wo)
    colt = T.im2col_t_ref(act.detach())
    w2 = wgt.permute(0, 2, 3, 1).reshape(co, 9 * c)  # (co, (kh, kw, c))
    assert close((w2 @ colt).view(co, b, ho, wo).permute(1, 0, 2, 3), out.detach())
    dout = torch.randn(b, co, ho, wo, generator=g, dtype=torch.float64)
    out.backward(dout)
    dcol = dout.permute(0, 2, 3, 1).reshape(b * ho * wo, co) @ w2
    assert close(T.col2im_relu_ref(dcol, torch.ones(b, h, w, c)), act.grad)
    gate = torch.randn(b, h, w, c, generator=g)
    assert close(T.col2im_relu_ref(dcol, gate), act.grad * (gate > 0))


def test_bn_finalize_ref_is_batchnorm():
    g = torch.Generator().manual_seed(6)
    n, C = 50, 12
    z = torch.randn(n, C, generator=g, dtype=torch.float64) * 2 + 1
    bn = torch.nn.BatchNorm1d(C, eps=T.f32(T.BN_EPS), momentum=T.f32(T.BN_MOMENTUM)).double().train()
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    bn.running_mean.copy_(rm)
    bn.running_var.copy_(rv)
    y = bn(z)
    sums = torch.stack([torch.cat([z[i::5].sum(0), (z[i::5] ** 2).sum(0)]) for i in range(5)])
    stats, nrm, nrv = T.bn_finalize_ref(sums, n, C, rm, rv)
    assert close((z - stats[:C]) * stats[C:], y.detach(), 1e-9)
    assert close(nrm, bn.running_mean) and close(nrv, bn.running_var)


def test_adam_ref_is_the_plain_loop():
    c = T.adam_case(9)
    hp = {k: T.f32(v) for k, v in c["hp"].items()}
    for i in range(9):
        p, g, m, v = (float(c[k][i]) for k in ("p", "g", "m", "v"))
        gi = g * hp["inv_scale"]
        m = hp["beta1"] * m + (1 - hp["beta1"]) * gi
        v = hp["beta2"] * v + (1 - hp["beta2"]) * gi * gi
        p = p - hp["lr_t"] * m / (math.sqrt(v) + hp["eps"])
        assert abs(p - float(c["pn"]["want"][i])) <= 1e-12 * max(abs(p), 1) and abs(m - float(c["mn"]["want"][i])) <= 1e-12
        assert abs(v - float(c["vn"]["want"][i])) <= 1e-12
    assert float(c["pn"]["want"][0]) == float(c["p"][0])  # v = g = m = 0: a step of exactly 0


# ---- every case: float32 passes, defects fail ------------------------------------------------------------------------------------------
def passes(result):
    worst, pos = result
    return worst <= 1 and not pos


ACT_GRID = [(act, x32, bwd, p, ss) for act in (T.ACT_SWISH, T.ACT_RELU) for x32 in (False, True) for bwd in (False, True)
            for p in T.DROP_PS + (T.P_TINY,) for ss in T.SEED_SALTS]


@pytest.mark.parametrize("act,x32,bwd,p,ss", ACT_GRID + [(T.ACT_SWISH, False, False, 0.0, T.SEED_SALTS[0])])
def test_act_dropout_cases(act, x32, bwd, p, ss):
    n = 1001 if x32 else 5 * 264
    c = T.act_dropout_case(n, act, p, ss[0], ss[1], x32, bwd)
    assert passes(T.check_drop_site(T.act_dropout_f32(c), c))
    if p in T.DROP_PS:
        wrong = T.keep_mask(ss[0], ss[1], np.arange(n, dtype=np.uint64), p, defect="mask_pair_swapped")
        assert not passes(T.check_drop_site(T.act_dropout_f32(c, keep=wrong), c))
        other = T.keep_mask(ss[0], ss[1] ^ 1, np.arange(n, dtype=np.uint64), p)  # the forward's salt in the backward, say
        assert not passes(T.check_drop_site(T.act_dropout_f32(c, keep=other), c))
    if p > 0:  # a kept value scaled by 1 / (1 - p) in the wrong place: after the rounding instead of before, or not at all
        noscale = dict(c, p=0.0)
        got = T.act_dropout_f32(noscale, keep=T.keep_mask(ss[0], ss[1], np.arange(n, dtype=np.uint64), p))
        assert not passes(T.check_drop_site(got, c)) or p == T.P_TINY and not x32  # (1e-5 is below half a bf16 step)
    if act == T.ACT_RELU and bwd:
        # relu_at_zero_passes has nothing to show here (|u| >= 2^-3); the subsampling cases carry the zeros
        assert float(c["u"].abs().min()) >= 2.0 ** -3


@pytest.mark.parametrize("cols", (256, 264))
@pytest.mark.parametrize("y_bf16", (False, True))
@pytest.mark.parametrize("p", T.DROP_PS + (T.P_TINY, 0.0))
def test_dropout_add_cases(cols, y_bf16, p):
    for (seed, salt), with_x in zip(T.SEED_SALTS, (True, False)):
        c = T.dropout_add_case(5, cols, y_bf16, with_x, p, seed, salt)
        assert passes(T.check_exact(c["want"], c))
        if p in T.DROP_PS:
            for d in ("mask_index_ld", "mask_pair_swapped"):
                bad = T.dropout_add_case(5, cols, y_bf16, with_x, p, seed, salt, ld=cols + 8, defect=d)
                assert not passes(T.check_exact(bad["want"], c)), d


@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("p", T.DROP_PS + (T.P_TINY, 0.0))
def test_dropout_bwd_cases(x32, p):
    for (seed, salt), cols in zip(T.SEED_SALTS, (256, 264)):
        c = T.dropout_bwd_case(5, cols, x32, p, seed, salt)
        assert bool((c["row_scale"] == 0).any())
        mid = c["lo"]
        assert bool((c["lo"] == c["hi"]).all()) and passes(T.check_drop_site(mid, c))
        defects = ("row_scale_missing",) + (("mask_index_ld", "mask_pair_swapped") if p in T.DROP_PS else ())
        for d in defects:
            bad = T.dropout_bwd_case(5, cols, x32, p, seed, salt, ld=cols + 8, defect=d)
            assert not passes(T.check_drop_site(bad["lo"], c)), d


LN_GRID = [(rows, D, dy_bf16, acc) for rows in T.LN_ROWS for D in T.LN_WIDTHS for dy_bf16 in (False, True) for acc in (False, True)
           if rows != 4099 or (dy_bf16, acc) in ((False, True), (True, False))]


@pytest.mark.parametrize("rows,D,dy_bf16,acc", LN_GRID)
def test_ln_bwd_cases(rows, D, dy_bf16, acc):
    c = T.ln_bwd_case(rows, D, dy_bf16, acc)
    assert passes(T.check_ln_bwd(T.ln_bwd_f32(c), c))
    for d in ("row_scale_missing", "partials_last_group_dropped"):
        if d == "row_scale_missing" and bool((c["row_scale"] == 1).all()):
            continue
        bad = T.ln_bwd_case(rows, D, dy_bf16, acc, defect=d)
        got = (bad["g"]["want"], bad["dgamma"]["want"], bad["dbeta"]["want"])
        assert not passes(T.check_ln_bwd(got, c)), d
    # the partials= form: the sums alone
    cp = dict(c, partials=True)
    assert passes(T.check_ln_bwd(T.ln_bwd_f32(cp), cp))
    # a reference with the variance over D - 1 (the mistake of every LayerNorm) is outside the bound
    x, rs = c["x"].double(), c["row_scale"].double()
    mu = x.mean(-1, keepdim=True)
    rstd_bad = 1 / torch.sqrt(((x - mu) ** 2).sum(-1, keepdim=True) / (D - 1) + T.f32(T.EPS_LN))
    w = c["dy"].double() * rs[:, None] * c["gamma"].double()
    xh = (x - mu) * rstd_bad
    gbad = (c["g0"].double() if c["accumulate"] else 0) + rstd_bad * (w - w.mean(-1, keepdim=True) - xh * (w * xh).mean(-1, keepdim=True))
    assert not passes(T.check_bound(gbad, c["g"]))


@pytest.mark.parametrize("D", T.LN_WIDTHS)
def test_ln_bwd_inplace_and_onehot(D):
    c = T.ln_bwd_case(5, D, False, False, inplace=True)
    assert passes(T.check_ln_bwd(T.ln_bwd_f32(c), c))
    rows = 4099
    for r in (0, rows - 1, 4097):  # the first row, the last row, a row of the wrapped round
        assert r == rows - 1 or r < 4096 or T.ln_last_round_rows(rows) == 4096
        c = T.ln_bwd_case(rows, D, True, True, onehot=r)
        got = T.ln_bwd_f32(c)
        assert passes(T.check_ln_bwd(got, c))
        if r >= 4096:
            bad = T.ln_bwd_case(rows, D, True, True, onehot=r, defect="partials_last_group_dropped")
            assert not passes(T.check_ln_bwd((got[0], bad["dgamma"]["want"], bad["dbeta"]["want"]), c))
        # a contribution of another row in dbeta, however small, fails the exact part
        leak = got[2].clone()
        leak[3] += 2.0 ** -20
        assert not passes(T.check_ln_bwd((got[0], got[1], leak), c))


def test_dy_next_cases():
    c = T.ln_bwd_case(5, 256, True, True)
    g_out = T.ln_bwd_f32(c)[0]
    rs2 = torch.tensor([1.0, 0.0, 1.0, 0.5, 1.0])
    for p in T.DROP_PS + (T.P_TINY, 0.0):
        for seed, salt in T.SEED_SALTS:
            w = T.dy_next_case(g_out, 0.5, rs2, p, seed, salt)
            assert bool((w["lo"] == w["hi"]).all()) and passes(T.check_drop_site(w["lo"], w))
            for d in ("row_scale_missing",) + (("mask_index_ld", "mask_pair_swapped") if p in T.DROP_PS else ()):
                bad = T.dy_next_case(g_out, 0.5, rs2, p, seed, salt, ld=264, defect=d)
                assert not passes(T.check_drop_site(bad["lo"], w)), d


@pytest.mark.parametrize("C", T.BN_CS)
@pytest.mark.parametrize("nparts", T.BN_NPARTS)
def test_bn_finalize_cases(nparts, C):
    c = T.bn_finalize_case(nparts, C)
    assert passes(T.check_bn_finalize(T.bn_finalize_f32(c), c))
    bad = T.bn_finalize_case(nparts, C, defect="bn_unbiased_in_rstd")
    assert not passes(T.check_bn_finalize((bad["stats"]["want"], bad["rm"]["want"], bad["rv"]["want"]), c))
    # the constant channel: variance exactly 0, rstd = 1 / sqrt(eps)
    assert abs(float(c["stats"]["want"][C + 1]) - 1 / math.sqrt(T.f32(T.BN_EPS))) < 1e-9
    # a group of partials left out (the remainder loop, or the last thread group)
    if nparts > 1:
        short = dict(c, sums=c["sums"][:-1])
        assert not passes(T.check_bn_finalize(T.bn_finalize_f32(short), c))


def test_bn_finalize_count_one():
    c = T.bn_finalize_case(1, 24, count=1)
    assert passes(T.check_bn_finalize(T.bn_finalize_f32(c), c))
    # every variance is 0 and count / max(count - 1, 1) = 1: the running variance decays towards 0, not towards NaN
    assert bool(torch.isfinite(c["rv"]["want"]).all()) and close(c["rv"]["want"], (1 - T.f32(T.BN_MOMENTUM)) * c["run_var"].double())


@pytest.mark.parametrize("shape", T.SUB_SHAPES)
@pytest.mark.parametrize("x32", (False, True))
def test_subsample_cases(shape, x32):
    c = T.subsample_case(shape, x32)
    b, h, w, ch = shape
    for d in ("relu_at_zero_passes", "col2im_even_edge"):
        if d == "col2im_even_edge" and h % 2 and w % 2:
            continue
        bad = T.subsample_case(shape, x32, defect=d)
        assert not passes(T.check_exact(bad["col2im"]["want"], c["col2im"])), d
    want = c["col2im"]["want"]
    if h % 2 == 0:
        assert float(want[:, h - 1].abs().max()) == 0.0
    if w % 2 == 0:
        assert float(want[:, :, w - 1].abs().max()) == 0.0
    # float32 restatement of col2im: exact on these integers
    got = T.col2im_relu_ref(c["dcol"], c["act"], dt=torch.float32) + 0.0
    assert passes(T.check_exact(got.to(want.dtype), c["col2im"]))
    r = T.relu_bwd_case(x32=x32)
    assert passes(T.check_exact(r["want"], r))
    assert not passes(T.check_exact(T.relu_bwd_case(x32=x32, defect="relu_at_zero_passes")["want"], r))


def test_convmid_fwd_ref_is_conv1d():
    g = torch.Generator().manual_seed(8)
    B, Tn, C, ks = 3, 21, 6, 7
    y = torch.randn(B * Tn, 2 * C, generator=g, dtype=torch.float64)
    w, bias = torch.randn(C, ks, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    s = F.glu(y.view(B, Tn, 2 * C), dim=-1).transpose(1, 2)
    want = F.conv1d(s, w[:, None, :], bias, padding=ks // 2, groups=C).transpose(1, 2).reshape(B * Tn, C)
    assert close(T.convmid_fwd_ref(y, B, Tn, C, w, bias)[0], want)


@pytest.mark.parametrize("Tn", T.CONV_TS)
@pytest.mark.parametrize("ks", T.CONV_KS)
def test_conv_forward_cases(ks, Tn):
    C = 256
    for x32 in (False, True):
        r = T.conv_route_case(ks, Tn, C, x32)
        z32, _ = T.convmid_fwd_ref(r["y"].float(), r["B"], Tn, C, r["w"], r["bias"], dt=torch.float32)
        assert passes(T.check_exact(z32, r))  # float32 with precise sigmoid: sigmoid(40) = 1, one rounding per element
        c = T.conv_random_case(ks, Tn, C, x32)
        z, bound = T.conv_z_bound(c)
        zc = {"want": z, "bound": bound}
        z32, _ = T.convmid_fwd_ref(c["y"].float(), c["B"], Tn, C, c["w"], c["bias"], dt=torch.float32)
        assert passes(T.check_bound(z32, zc))
        for d in ("taps_flipped", "halo_crosses_utterance", "last_strip_dropped"):
            if d == "last_strip_dropped" and Tn % 16 == 0 or d == "taps_flipped" and Tn == 1:
                continue  # (one frame: only the centre tap is ever used)
            bad, _ = T.convmid_fwd_ref(c["y"].float(), c["B"], Tn, C, c["w"], c["bias"], defect=d)
            assert not passes(T.check_bound(bad, zc)), d
            assert not passes(T.check_exact(T.conv_route_case(ks, Tn, C, x32, defect=d)["want"], r)), d
        # the partial sums: compensated float32 sums of 32-frame groups pass, a plain float32 chain or sums that miss the last
        # strip's frames do not
        zf = z32.float()
        sb = T.conv_sums_bound(zf, c["B"], Tn, C)
        parts = part_sums(zf.view(c["B"], Tn, C))
        assert passes(T.check_bound(parts.double().sum(0), sb))
        if Tn % 16:
            keep = torch.ones(c["B"], Tn, 1)
            keep[:, Tn // 16 * 16:] = 0
            zs = zf * keep.view(-1, 1)
            assert not passes(T.check_bound(torch.cat([zs.double().sum(0), (zs.double() ** 2).sum(0)]), sb))


def test_conv_backward_refs_are_autograd():
    g = torch.Generator().manual_seed(9)
    B, Tn, C, ks = 3, 21, 6, 7
    y = torch.randn(B * Tn, 2 * C, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(C, ks, generator=g, dtype=torch.float64).requires_grad_()
    bias = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    z, _ = T.convmid_fwd_ref(y, B, Tn, C, w, bias)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    stats = torch.cat([mean, 1 / torch.sqrt(var + 1e-5)])
    nv = gamma * (z - mean) * stats[C:] + beta
    out = nv * torch.sigmoid(nv)
    dout = torch.randn(B * Tn, C, generator=g, dtype=torch.float64)
    out.backward(dout)
    dn, dsum, dz, _ = T.bn_swish_bwd_ref(dout, z.detach(), stats.detach(), gamma.detach(), beta.detach())
    assert close(dsum[:C], beta.grad) and close(dsum[C:], gamma.grad)
    dy, dw, db = T.convmid_bwd_ref(dz, y.detach(), B, Tn, C, w.detach())
    assert close(dy, y.grad, 1e-9) and close(dw, w.grad, 1e-9)
    assert float(db.abs().max()) < 1e-9 and float(bias.grad.abs().max()) < 1e-9  # the bias feeds a BatchNorm: its gradient is zero
    # db itself: the plain sum of a dz that is not a BatchNorm's
    dz2 = torch.randn(B * Tn, C, generator=g, dtype=torch.float64)
    z2, _ = T.convmid_fwd_ref(y, B, Tn, C, w, bias)
    y.grad = w.grad = bias.grad = None
    z2.backward(dz2)
    dy, dw, db = T.convmid_bwd_ref(dz2, y.detach(), B, Tn, C, w.detach())
    assert close(dy, y.grad) and close(dw, w.grad) and close(db, bias.grad)


@pytest.mark.parametrize("rows", T.BN_BWD_ROWS)
def test_bn_swish_bwd_cases(rows):
    for C, x32 in ((256, False), (256, True), (768, False)):
        c = T.bn_swish_bwd_case(rows, C, x32)
        for name, got in zip(("dn", "dsum", "dz"), T.bn_swish_bwd_f32(c)):
            assert passes(T.check_bound(got, c[name])), name
        if rows > 1:
            bad = T.bn_swish_bwd_f32(c, defect="dsum_not_divided")
            assert not passes(T.check_bound(bad[2], c["dz"]))
            assert not passes(T.check_bound(T.bn_swish_bwd_case(rows, C, x32, defect="dsum_not_divided")["dz"]["want"], c["dz"]))
        # a row left out of the sums (the wrapped round at 1030 rows, or the last row group)
        if rows > 1:
            short = dict(c, dout=c["dout"][:-1], z=c["z"][:-1])
            assert not passes(T.check_bound(T.bn_swish_bwd_f32(short)[1], c["dsum"]))
    r = rows - 1
    c = T.bn_swish_bwd_case(rows, 256, False, onehot=r)
    dn, dsum, _ = T.bn_swish_bwd_f32(c)
    assert torch.equal(dsum[:256], dn[r])  # one-hot dout: dsum is that row's dn exactly


@pytest.mark.parametrize("Tn", T.CONV_TS)
@pytest.mark.parametrize("ks", T.CONV_KS)
def test_conv_backward_cases(ks, Tn):
    C = 256
    for x32 in (False, True):
        c = T.conv_bwd_random_case(ks, Tn, C, x32)
        dy, dw, db = T.convmid_bwd_f32(c)
        assert passes(T.check_conv_dy(dy, c["dy"])) and passes(T.check_bound(dw, c["dw"]))
        assert passes(T.check_bound(db, c["db"]))
        for d in ("taps_flipped", "halo_crosses_utterance", "last_strip_dropped"):
            if d == "last_strip_dropped" and Tn % 16 == 0 or d == "taps_flipped" and Tn == 1:
                continue
            bdy, bdw, bdb = T.convmid_bwd_f32(c, defect=d)
            assert not passes(T.check_conv_dy(bdy, c["dy"])), d
            assert not passes(T.check_bound(bdw, c["dw"])) or Tn == 1, d
    pad = (ks - 1) // 2
    caught = set()
    for t0, t1, b0, b1 in T.conv_bwd_routes(Tn):
        r = T.conv_bwd_route_case(ks, Tn, C, t0, t1, b0, b1)
        got = T.convmid_bwd_ref(r["dz"], r["y"], 3, Tn, C, r["w"], dt=torch.float32)
        for name, t in zip(("dy", "dw", "db"), got):
            assert passes(T.check_exact((t + 0.0).float(), r[name])), name
        j = t1 - t0 + pad
        want = r["dw"]["want"]
        if b0 == b1 and 0 <= j < ks:
            assert float(want[0, j]) == 8.0 and float(want.abs().sum()) == 8.0 * C
        else:
            assert float(want.abs().sum()) == 0.0
        assert float(r["dy"]["want"].view(3, Tn, 2 * C)[[b for b in range(3) if b != b0]].abs().sum()) == 0.0
        for d in ("taps_flipped", "halo_crosses_utterance"):
            bad = T.conv_bwd_route_case(ks, Tn, C, t0, t1, b0, b1, defect=d)
            if not all(torch.equal(bad[k]["want"], r[k]["want"]) for k in ("dy", "dw")):
                caught.add(d)
    # over the routes, each defect shows (one frame: only the centre tap exists, nothing to flip)
    assert caught == ({"halo_crosses_utterance"} if Tn == 1 else {"taps_flipped", "halo_crosses_utterance"}), caught


def test_conv1_dw_ref_is_conv2d_autograd():
    g = torch.Generator().manual_seed(10)
    b, t, idim, c = 2, 9, 11, 5
    x = torch.randn(b, t, idim, generator=g, dtype=torch.float64)
    mean, istd = torch.randn(idim, generator=g, dtype=torch.float64), 0.5 + torch.rand(idim, generator=g, dtype=torch.float64)
    h1, w1 = T.out_hw(t, idim)
    dact = torch.randn(b * h1 * w1, c, generator=g, dtype=torch.float64)
    wgt = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    o = F.conv2d(((x - mean) * istd)[:, None], wgt, bias, stride=2)
    o.backward(dact.view(b, h1, w1, c).permute(0, 3, 1, 2))
    dw, db = T.conv1_dw_ref(dact, x, mean, istd)
    assert close(dw, wgt.grad.view(c, 9)) and close(db, bias.grad)


@pytest.mark.parametrize("shape", T.CONV1_SHAPES)
def test_conv1_dw_cases(shape):
    for x32 in (False, True):
        for cmvn in (False, True):
            c = T.conv1_dw_case(shape, x32, cmvn)
            assert passes(T.check_conv1_dw(T.conv1_dw_f32(c), c))
            assert not passes(T.check_conv1_dw(T.conv1_dw_f32(c, transposed=True), c))
            # the positions of the last strip (npos % 64 of them) left out
            b, t, idim, ch = shape
            h1, w1 = T.out_hw(t, idim)
            npos = b * h1 * w1
            if npos % 64:
                short = dict(c, dact=torch.cat([c["dact"][:npos // 64 * 64], torch.zeros_like(c["dact"][npos // 64 * 64:])]))
                assert not passes(T.check_conv1_dw(T.conv1_dw_f32(short), c))


def test_epilogue_layernorm_backward_cases():
    """dense_join_splitk, dense_lnbwd and ffn_train_bwd: float32 restatements pass, planted defects fail."""
    for p in T.DROP_PS + (0.0,):
        seed, salt = T.SEED_SALTS[0]
        c = T.dense_join_case(T.SPLITK_K, p, seed, salt, with_rs=False)
        assert passes(T.check_exact(c["want"], c)) and bool((c["row_scale"] == 1).all())
        for d in ("mask_index_ld", "mask_pair_swapped") if p else ():
            assert not passes(T.check_exact(T.dense_join_case(T.SPLITK_K, p, seed, salt, with_rs=False, defect=d)["want"], c)), d
    c = T.dense_lnbwd_case()
    g32, dg, db, _ = T.ln_bwd_ref(c["x"], c["gamma"], c["dy"], c["g0"], c["row_scale"], True, dt=torch.float32)
    assert passes(T.check_ln_bwd((g32, dg.double(), db.double()), c))
    bad = T.dense_lnbwd_case(defect="row_scale_missing")
    assert not passes(T.check_ln_bwd((bad["g"]["want"], bad["dgamma_sum"]["want"], bad["dbeta_sum"]["want"]), c))
    # ffn_train_bwd reads the tape: du follows the tape's mask bit for bit, a tape made with another salt gives another du
    fc = T.ffn_train_case(0.1, 0.1, 77, 3, 4)
    bc = T.ffn_bwd_case()
    gk = fc["gk"]["lo"]
    du, ln = T.ffn_bwd_want(bc, gk)
    g32, dg, db, _ = T.ln_bwd_ref(ln["x"], ln["gamma"], ln["dy"], ln["g0"], None, True, dt=torch.float32)
    assert passes(T.check_ln_bwd((g32, dg.double(), db.double()), ln))
    assert bool(((du.float() == 0) == ((gk.float() == 0) | (bc["dh"] == 0))).all())
    other = T.ffn_train_case(0.1, 0.1, 77, 5, 4)["gk"]["lo"]
    du2, ln2 = T.ffn_bwd_want(bc, other)
    assert not passes(T.check_exact(du2, {"want": du})) and not passes(T.check_bound(ln2["g"]["want"], ln["g"]))


def part_sums(zf):
    """(B, T, C) float32 -> the (sum | sum of squares) partial vectors of 32-frame groups as a compensated float32 sum leaves them:
    the correctly rounded sum of the float32 terms (squares rounded to float32 first)."""
    B, Tn, _ = zf.shape
    sq = (zf * zf)
    return torch.stack([torch.cat([zf[b, t0:t0 + 32].double().sum(0), sq[b, t0:t0 + 32].double().sum(0)]).float()
                        for b in range(B) for t0 in range(0, Tn, 32)])


def test_bn_onepass_case():
    """The one-pass variance with |mean| / sigma in {0, 4, 32}: compensated float32 partials finalized in double pass the derived
    bound, whose relative error of rstd at ratio 32 over 64 x 255 frames is BELOW 2^-9 (half a bf16 step of the normalised
    activations); the former arithmetic - plain float32 chains and a float32 subtraction - is outside it."""
    C = 256
    ratio = torch.tensor([0.0, 4.0, 32.0])[torch.arange(C) % 3]
    for B, Tn in ((3, 47), (64, 255)):
        c = T.conv_random_case(15, Tn, C, False, B=B, bias_ratio=ratio)
        z32, _ = T.convmid_fwd_ref(c["y"].float(), B, Tn, C, c["w"], c["bias"], dt=torch.float32)
        zf = z32.float().view(B, Tn, C)
        parts = part_sums(zf)
        oc = T.bn_onepass_case(parts, zf.view(-1, C), B * Tn, C)
        got = T.bn_finalize_f32(dict(oc, sums=parts))
        assert passes(T.check_bn_finalize(got, oc))
        rel = oc["stats"]["bound"][C:] / oc["stats"]["want"][C:]
        assert float(rel.max()) < 2.0 ** -9
        # plain float32: sequential chains in the workgroup and in the finalize, the subtraction in float32
        chain = torch.zeros(2 * C)
        for b in range(B):
            for t0 in range(0, Tn, 32):
                a = torch.zeros(2 * C)
                for t in range(t0, min(t0 + 32, Tn)):
                    a = a + torch.cat([zf[b, t], zf[b, t] * zf[b, t]])
                chain = chain + a
        old = T.bn_finalize_ref(chain[None, :], B * Tn, C, oc["run_mean"], oc["run_var"], dt=torch.float32)
        print(B, Tn, "the former float32 arithmetic: error / bound", T.check_bn_finalize(old, oc)[0])
        if Tn == 255:
            assert not passes(T.check_bn_finalize(old, oc))


@pytest.mark.parametrize("act,bwd", ((T.ACT_RELU, False), (T.ACT_RELU, True), (T.ACT_SWISH, False), (T.ACT_SWISH, True)))
def test_dense_act_cases(act, bwd):
    for p in T.DROP_PS + (0.0,):
        seed, salt = T.SEED_SALTS[0]
        c = T.dense_act_case(act, bwd, p, seed, salt)
        assert passes(T.check_drop_site(T.dense_act_f32(c), c))
        for d in ("mask_index_ld", "mask_pair_swapped") if p else ():
            assert not passes(T.check_drop_site(T.dense_act_f32(c, defect=d), c)), d
    if act == T.ACT_RELU and bwd:  # u holds zeros here
        c = T.dense_act_case(act, bwd, 0.1, 1, 2)
        bad = T.dense_act_case(act, bwd, 0.1, 1, 2, defect="relu_at_zero_passes")
        assert bool((c["u"] == 0).any()) and not passes(T.check_drop_site(bad["lo"], c))


@pytest.mark.parametrize("k", (256, 512))
def test_dense_join_cases(k):
    for p in T.DROP_PS + (0.0,):
        seed, salt = T.SEED_SALTS[1]
        c = T.dense_join_case(k, p, seed, salt)
        assert passes(T.check_exact(c["want"], c))
        for d in ("row_scale_missing",) + (("mask_index_ld", "mask_pair_swapped") if p else ()):
            assert not passes(T.check_exact(T.dense_join_case(k, p, seed, salt, defect=d)["want"], c)), d


def test_ffn_train_cases():
    seed, sh, sj = 77, 3, 4
    for p in T.DROP_PS:
        c = T.ffn_train_case(p, p, seed, sh, sj)
        u = c["u"].float()
        keep = torch.from_numpy(T.keep_mask(seed, sh, T.site_index(c["m"], c["hidden"]), p))
        ik = torch.tensor(float(T.drop_params(p)[1]))
        h = T.bf16_rne(torch.where(keep, T.act_fwd_ref(u, T.ACT_SWISH, dt=torch.float32) * ik, torch.zeros_like(u)))
        gk = T.bf16_rne(torch.where(keep, T.act_grad_ref(u, T.ACT_SWISH, dt=torch.float32) * ik, torch.zeros_like(u)))
        assert passes(T.check_drop_site(h, c["h"])) and passes(T.check_drop_site(gk, c["gk"]))
        want = T.ffn_join_want(c, h)
        for d in ("mask_index_ld", "mask_pair_swapped"):
            bad = T.ffn_train_case(p, p, seed, sh, sj, defect=d)
            assert not passes(T.check_drop_site(bad["h"]["lo"], c["h"])) and not passes(T.check_drop_site(bad["gk"]["lo"], c["gk"])), d
            assert not passes(T.check_exact(T.ffn_join_want(c, h, defect=d)["want"], want)), d
        # the hidden site's salt at the join (or the reverse) is a different mask
        swapped = dict(c, salt_join=sh)
        assert not passes(T.check_exact(T.ffn_join_want(swapped, h)["want"], want))


@pytest.mark.parametrize("C", T.CONV_CS)
@pytest.mark.parametrize("x32", (False, True))
def test_bn_swish_fwd_cases(C, x32):
    c = T.bn_swish_fwd_case(141, C, x32)
    got = T.bn_swish_fwd_f32(c)
    assert passes(T.check_bn_swish_out(got, c, cap=T.BN_OUT_CAP_F32))  # the bf16 cap of the float32 restatement: 0.05 %
    # the running instead of the batch statistics, or gamma and beta exchanged: outside
    wrong = dict(c, gamma=c["beta"], beta=c["gamma"])
    assert not passes(T.check_bn_swish_out(T.bn_swish_fwd_f32(wrong), c))
    # a channel index off by one row stride (c = i % (C + 1)) shows in the first row already
    shifted = dict(c, stats=torch.roll(c["stats"], 1))
    assert not passes(T.check_bn_swish_out(T.bn_swish_fwd_f32(shifted), c))
    if not x32:  # bf16 by truncation: far above the cap
        nv = c["gamma"] * (c["z"] - c["stats"][:C]) * c["stats"][C:] + c["beta"]
        assert not passes(T.check_bn_swish_out(T.G.truncate_bf16(nv * torch.sigmoid(nv)), c))


@pytest.mark.parametrize("n", (1, 4, 1001))
def test_adam_cases(n):
    c = T.adam_case(n)
    c["mirror0"] = torch.zeros(n, dtype=torch.bfloat16)
    assert passes(T.check_adam(T.adam_f32(c, mirror=True), c))
    if n > 1:
        assert not passes(T.check_adam(T.adam_f32(c, mirror=True, defect="mirror_truncates"), c))
    assert bool(torch.isfinite(c["pn"]["want"]).all())
    o = T.adam_case(n, overflow=1)
    o["mirror0"] = T.bf16_rne(o["p"])
    assert passes(T.check_adam(T.adam_f32(o, mirror=True), o))
    if n > 1:  # (element 0 has g = m = v = 0: its update is the identity)
        assert not passes(T.check_adam(T.adam_f32(o, mirror=True, defect="adam_ignores_overflow"), o))


def test_adam_mirror_ties():
    c = T.adam_case(64, lr_t=0.0)
    assert bool(G_is_tie(c["p"]).all())
    c["mirror0"] = torch.zeros(64, dtype=torch.bfloat16)
    got = T.adam_f32(c, mirror=True)
    assert torch.equal(got[0], c["p"]) and passes(T.check_adam(got, c))
    upper = c["p"].view(torch.int32) >> 16
    assert bool((upper & 1).bool().any()) and bool(((upper & 1) == 0).any())  # ties that round up and ties that round down
    assert not passes(T.check_adam(T.adam_f32(c, mirror=True, defect="mirror_truncates"), c))


def G_is_tie(x):
    return T.G.is_tie(x)


def test_overflow_ref():
    g = torch.zeros(8)
    g[3] = torch.finfo(torch.float32).max
    g[4] = 2.0 ** -149
    assert T.overflow_ref(g) == 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        h = g.clone()
        h[7] = bad
        assert T.overflow_ref(h) == 1


def test_defect_list_is_covered():
    """Every name the issue lists is in DEFECTS, and a reference of this module plants each (a defect nobody plants proves nothing):
    the planted result differs from the correct one."""
    issue = ("mask_index_ld", "mask_pair_swapped", "taps_flipped", "halo_crosses_utterance", "last_strip_dropped", "row_scale_missing",
             "partials_last_group_dropped", "bn_unbiased_in_rstd", "dsum_not_divided", "relu_at_zero_passes", "col2im_even_edge",
             "adam_ignores_overflow", "mirror_truncates")
    assert set(issue) == set(T.DEFECTS)
    idx = np.arange(4096, dtype=np.uint64)
    o = T.adam_case(8, overflow=1)
    o["mirror0"] = T.bf16_rne(o["p"])
    cb = T.conv_bwd_random_case(7, 17, 256, True)
    sb = T.bn_swish_bwd_case(7, 256)
    planted = {
        "mask_index_ld": lambda d: not torch.equal(T.site_index(5, 256, 264, d), T.site_index(5, 256, 264)),
        "mask_pair_swapped": lambda d: bool((T.keep_mask(1, 2, idx, 0.5, d) != T.keep_mask(1, 2, idx, 0.5)).any()),
        "taps_flipped": lambda d: not torch.equal(T.convmid_bwd_f32(cb, d)[1], T.convmid_bwd_f32(cb)[1]),
        "halo_crosses_utterance": lambda d: not torch.equal(T.convmid_bwd_f32(cb, d)[0], T.convmid_bwd_f32(cb)[0]),
        "last_strip_dropped": lambda d: not torch.equal(T.convmid_bwd_f32(cb, d)[0], T.convmid_bwd_f32(cb)[0]),
        "row_scale_missing": lambda d: not torch.equal(T.ln_bwd_case(5, 256, False, True, defect=d)["g"]["want"],
                                                         T.ln_bwd_case(5, 256, False, True)["g"]["want"]),
        "partials_last_group_dropped": lambda d: not torch.equal(T.ln_bwd_case(5, 256, False, True, defect=d)["dbeta"]["want"],
                                                                   T.ln_bwd_case(5, 256, False, True)["dbeta"]["want"]),
        "bn_unbiased_in_rstd": lambda d: not torch.equal(T.bn_finalize_case(17, 16, defect=d)["stats"]["want"],
                                                           T.bn_finalize_case(17, 16)["stats"]["want"]),
        "dsum_not_divided": lambda d: not torch.equal(T.bn_swish_bwd_f32(sb, d)[2], T.bn_swish_bwd_f32(sb)[2]),
        "relu_at_zero_passes": lambda d: not torch.equal(T.relu_bwd_case(defect=d)["want"], T.relu_bwd_case()["want"]),
        "col2im_even_edge": lambda d: not torch.equal(T.subsample_case(T.SUB_SHAPES[1], defect=d)["col2im"]["want"],
                                                        T.subsample_case(T.SUB_SHAPES[1])["col2im"]["want"]),
        "adam_ignores_overflow": lambda d: not torch.equal(T.adam_f32(o, defect=d)[0], T.adam_f32(o)[0]),
        "mirror_truncates": lambda d: not torch.equal(T.store_round(o["p"], torch.bfloat16, d), T.store_round(o["p"], torch.bfloat16)),
    }
    for d in T.DEFECTS:
        assert planted[d](d), d
