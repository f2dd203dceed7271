"""CPU: the conditions the exact ECAPA cases of tests/ecapa_cases.py rest on, asserted on the references alone, and the proof that
the comparators of test_ecapa_exact_gpu.py reject the defects these kernels could have - each defect is applied to the reference
and handed to the comparator in place of a device output.  The defects marked (+) are also handed to the whole-tensor tolerance of
tests/test_ecapa_gpu.py on that test's own random operands, at the mildest site the defect can sit at (one channel, one wave, a
zero-filled buffer): it accepts them.  Two defects the issue lists among those are NOT accepted by that tolerance and the tests say
so instead of pretending: a keep mask one row late moves a whole output row into the halo (the old test rejects it by its max-error
term and its halo check), and the uniformly weighted first tile is rejected by the entry point's own old tolerance at T = 300 -
what accepts it is the model-level tolerance of test_ecapa_forward_matches_oracle, which is what is asserted here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecapa_cases as E  # noqa: E402
import gemm_cases as G  # noqa: E402

BF16 = torch.bfloat16


def _window_with(want, got=None, canary_rows=()):
    """A bf16 Window holding `got` (default: want) with the listed rows left as canaries; returns check_window's message."""
    M, N = want.shape
    win = G.Window(M, N, BF16, "a8").snapshot()
    win.view.copy_(want if got is None else got)
    for r in canary_rows:
        G._bits(win.view)[r] = G.BF16_CANARY
    return G.check_window(win, want, (16, 32))


# ---- Res2Net ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", E.R2_CCS)
@pytest.mark.parametrize("shape", E.R2_SHAPES, ids=lambda s: "T%d_H%d_d%d" % s)
def test_res2net_case_conditions(cc, shape):
    T, H, d = shape
    c = E.Res2Case(cc, T, H, d, seed=T + cc)
    stats = {}
    y = c.ref(stats=stats)
    print("cc %d T %d H %d d %d: margin %.4f, |y| <= %g, non-zero %.2f .. %.2f, rounded y %.3f, rounded x + y %.3f" % (
        cc, T, H, d, stats["margin"], stats["ymax"], min(stats["nonzero"]), max(stats["nonzero"]), stats["round_y"], stats["round_add"]))
    assert stats["margin"] < 1
    assert min(stats["nonzero"]) >= 0.5
    if stats["count"] >= 1000:
        # y = bf16(...) changes >= 5 % of the elements.  bf16(x + y) cannot reach that share with these operands: y is a bf16 number
        # and x an integer of -2 .. 2, so the sum needs a ninth bit only where it climbs into the next binade with an odd last bit
        # (measured: 0.7 .. 1.2 % of the elements on every case); what is asserted is that the case has hundreds of such elements
        # and that the comparator sees the defect that skips this rounding (test_res2net_defects_are_rejected[add_f32]).
        assert stats["round_y"] >= 0.05
        assert stats["round_add"] >= 0.005 and stats["round_add"] * stats["count"] * 6 >= 50
    assert bool((y[:, :H, cc:] == 0).all()) and bool((y[:, H + T:, cc:] == 0).all())
    assert torch.equal(y[..., :cc], c.x.double()[..., :cc])
    assert bool((c.x[:, :H] == 0).all()) and bool((c.x[:, H + T:] == 0).all())
    assert not torch.equal(y[0], y[1]) and not torch.equal(y[1], y[2])
    assert int((c.w != 0).sum(-1).min()) >= 4 and int((c.w != 0).sum(-1).max()) <= 8
    assert bool((c.shift[1:] != c.shift[:-1]).all())
    assert E.rne(y).equal(y)  # every value of the reference is a bf16 number


def _old_res2_data(cc=64, b=2, t=20, d=3, H=4):
    """The operands of test_ecapa_gpu.py::test_res2net_fused_entry_point_against_float64."""
    g = torch.Generator().manual_seed(1000 * cc + 10 * t + d)
    c, tp = 8 * cc, t + 2 * H
    x = torch.zeros(b, tp, c)
    x[:, H:H + t] = torch.randn(b, t, c, generator=g)
    w = (torch.randn(7, cc, 3 * cc, generator=g) / (3 * cc) ** 0.5).bfloat16()
    bias, sc, sh = torch.randn(7, cc, generator=g) * 0.1, torch.rand(7, cc, generator=g) + 0.5, torch.randn(7, cc, generator=g) * 0.1
    return [v.double() for v in (x.bfloat16(), w, bias, sc, sh)] + [t, H, d]


@pytest.mark.parametrize("defect", E.R2_DEFECTS)
def test_res2net_defects_are_rejected(defect):
    c = E.Res2Case(64, 9, 4, 1, seed=5) if defect == "drop_last_row" else E.Res2Case(64, 40, 4, 3, seed=5)
    want = c.ref().view(-1, c.C).bfloat16()
    assert _window_with(want) is None
    if defect == "drop_last_row":
        rows = [b * c.tp + c.tp - 1 for b in range(c.B)]
        win = G.Window(want.shape[0], c.C, BF16, "a8").snapshot()
        win.view.copy_(want)
        for r in rows:
            G._bits(win.view)[r, c.cc:] = G.BF16_CANARY
        assert G.check_window(win, want, (16, 32)) is not None
    else:
        for site in ((0, 17, c.cc - 1) if defect == "prev_params" else (None,)):
            got = c.ref(defect=defect, site=site).view(-1, c.C).bfloat16()
            assert _window_with(want, got) is not None, (defect, site)


@pytest.mark.parametrize("defect", ("prev_params", "drop_last_row", "add_f32"))
def test_res2net_defects_the_old_tolerance_accepts(defect):
    """(+) on the old test's operands: prev_params at the channel of step 7 whose step-6 parameters are closest, drop_last_row into
    that test's zero-filled buffer, add_f32 everywhere."""
    x, w, bias, sc, sh, t, H, d = _old_res2_data()
    want = E.res2net_ref(x, w, bias, sc, sh, t, H, d)
    if defect == "drop_last_row":
        got = E.drop_last_row(want, 0.0, 64)
        assert E.res2_old_check(got, want, H, t)
    elif defect == "add_f32":
        got = E.res2net_ref(x, w, bias, sc, sh, t, H, d, defect=defect)
        assert not torch.equal(got, want) and E.res2_old_check(got, want, H, t)
    else:
        dist = (bias[6] - bias[5]).abs() + (sc[6] - sc[5]).abs() * 2 + (sh[6] - sh[5]).abs()
        site = int(dist.argmin())
        got = E.res2net_ref(x, w, bias, sc, sh, t, H, d, defect=defect, site=site)
        assert not torch.equal(got, want) and E.res2_old_check(got, want, H, t)


def test_res2net_keep_mask_one_row_late_is_rejected_by_both():
    """Not (+) after all: the late mask zeroes frame 0 and lets a full row into the halo - beyond 4 % of the maximum, and the old
    test also looks at the halo rows."""
    x, w, bias, sc, sh, t, H, d = _old_res2_data()
    want = E.res2net_ref(x, w, bias, sc, sh, t, H, d)
    got = E.res2net_ref(x, w, bias, sc, sh, t, H, d, defect="keep_late")
    assert not E.res2_old_check(got, want, H, t)
    assert float((got - want).abs().max()) > 4e-2 * float(want.abs().max())


# ---- ASP -------------------------------------------------------------------------------------------------------------------------------
ASP_ALL = [(s, True) for s in E.ASP_FUSED_SHAPES] + [(s, False) for s in E.ASP_POOL8_SHAPES + E.ASP_SCALAR_SHAPES]


@pytest.mark.parametrize("shape,fused", ASP_ALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("fused" if v else "pool"))
def test_asp_selector_conditions(shape, fused):
    B, T, C = shape
    c = E.AspCase(B, T, C, fused=fused)
    k = c.conditions()
    print(shape, "fused" if fused else "pool", k)
    assert k["levels"] and k["n_ok"]
    assert k["frame0"] and k["frame_last"] and k["boundaries"]
    if fused:
        assert set(k["want_tiles"]) <= set(k["first_tiles"])
    if T >= 15:
        assert k["n_kinds"] == [1, 2, 4] and (k["lanes_unseen"] or not fused)
    assert T * 64 * 2 < 2 ** 24  # |x| <= 8: every sum of w x^2 is an integer far below 2^24
    inner = c.x[:, c.H:c.H + T].double()
    assert float(inner.abs().max()) <= 8 and bool((c.x[:, :c.H] == E.POISON).all()) and bool((c.x[:, c.H + T:] == E.POISON).all())
    assert bool((c.logits64()[:, :c.H] == 0).all())  # halo rows would select
    out, parts = c.ref()
    n = c.sel.sum(1).double()
    assert torch.equal(parts["s0"], n)
    # exact statistics: S1 / n and S2 / n on a 1/4 lattice, the mean half of the output a bf16 number
    assert bool((parts["mean"] * 4 == (parts["mean"] * 4).round()).all()) and bool((parts["ex2"] * 4 == (parts["ex2"] * 4).round()).all())
    assert torch.equal(E.rne(out[:, :C]), out[:, :C])
    one = n == 1
    assert bool((parts["var"][one] == E.EPS32).all())
    bound = E.std_bound(out, parts)
    share = E.multi_share(out, bound)
    print("intervals wider than one bf16 number: %.4f" % share)
    assert share <= 0.02
    assert bool((c.sc[:C] != c.sc[C:]).all()) and bool((c.sh[:C] != c.sh[C:]).all())


def _asp_rejected(c, defect, site=None):
    out, parts = c.ref()
    bad, _ = c.ref(defect=defect, site=site)
    bound = E.std_bound(out, parts)
    assert bool(E.in_interval(out.float().bfloat16(), out, bound).all())
    return not bool(E.in_interval(bad.float().bfloat16(), out, bound).all())


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("defect", E.ASP_DEFECTS)
def test_asp_defects_are_rejected(defect, fused):
    c = E.AspCase(2, 65, 256, fused=True) if fused else E.AspCase(2, 70, 192, fused=False)
    sites = {"swap": [(0, 1), (37, 44), (c.C - 2, c.C - 1)], "std_mean_params": [0, 5, c.C - 1]}.get(defect, [None])
    for site in sites:
        assert _asp_rejected(c, defect, site), (defect, site)


def _old_asp_data(b=1, t=1, c=256, H=4):
    g = torch.Generator().manual_seed(100 * t + c)
    tp = t + 2 * H
    a1 = torch.tanh(torch.randn(b, tp, 128, generator=g)).bfloat16()
    w = (torch.randn(c, 128, generator=g) * 0.3).bfloat16()
    x = torch.randn(b, tp, c, generator=g).bfloat16()
    sc, sh = torch.rand(2 * c, generator=g) + 0.5, torch.randn(2 * c, generator=g) * 0.1
    return a1.double() @ w.double().T, x.double(), sc.double(), sh.double(), t, H


@pytest.mark.parametrize("defect", ("swap", "std_mean_params"))
def test_asp_defects_the_old_tolerance_accepts(defect):
    """(+) on the old test's operands at (1, 1, 256): some pair of channels of one 16-channel group / some channel has statistics
    similar enough for 2 % of the maximum + 1e-2."""
    lf, x, sc, sh, t, H = _old_asp_data()
    want, _ = E.asp_ref(lf, x, sc, sh, t, H, eps=1e-12)
    C = x.shape[2]
    sites = [(a, b) for g0 in range(0, C, 16) for a in range(g0, g0 + 16) for b in range(a + 1, g0 + 16)] if defect == "swap" else range(C)
    accepted = 0
    for site in sites:
        got, _ = E.asp_ref(lf, x, sc, sh, t, H, eps=1e-12, defect=defect, site=site)
        assert not torch.equal(got, want)
        accepted += E.asp_old_check(got, want)
    print(defect, "accepted at", accepted, "of", len(sites), "sites")
    assert accepted >= 1


def test_asp_uniform_first_tile_passes_the_model_level_tolerance():
    """(+) the historical defect (the first 16 frames weighted as the maximum) inside the oracle model at (2, 300), C = 512, held
    to the model-level tolerance of test_ecapa_forward_matches_oracle; the entry point's own old tolerance rejects it at T = 300."""
    from oracle import ecapa_oracle as O

    torch.manual_seed(3)
    ref = O.EcapaTDNN(80, channels=(512, 512, 512, 512, 1536)).eval()
    x = torch.randn(2, 300, 80)

    def defective(z):
        l = ref.asp.conv(torch.tanh(ref.asp.tdnn(z)))
        l = torch.cat([l.max(2, keepdim=True).values.expand(-1, -1, 16), l[:, :, 16:]], 2)
        w = torch.softmax(l, dim=2)
        mean = (w * z).sum(2)
        std = torch.sqrt((w * (z - mean.unsqueeze(2)) ** 2).sum(2).clamp(min=1e-12))
        return torch.cat((mean, std), dim=1).unsqueeze(2)

    with torch.no_grad():
        want = ref(x)
        ref.asp.forward = defective
        got = ref(x)
    rel = float((got - want).norm() / want.norm())
    cos = float(torch.nn.functional.cosine_similarity(got, want, dim=1).min())
    print("uniform first tile in the model: rel %.3e, cos %.6f" % (rel, cos))
    assert not torch.equal(got, want) and rel < 3e-2 and cos > 0.999
    lf, xx, sc, sh, t, H = _old_asp_data(2, 300, 256)
    w_, _ = E.asp_ref(lf, xx, sc, sh, t, H, eps=1e-12)
    g_, _ = E.asp_ref(lf, xx, sc, sh, t, H, eps=1e-12, defect="uniform16")
    assert not E.asp_old_check(g_, w_)


@pytest.mark.parametrize("fused,offset", [(True, 0.0), (True, 16.0), (False, 0.0), (False, 16.0)])
def test_asp_bounded_case_reference(fused, offset):
    """The bound is no blanket: it stays below a bf16 step of the output for most elements without the offset, and the float32
    emulation (float32 products and sums of the float64 weights) sits inside it."""
    c = E.AspRandomCase(2, 130, 256, fused=fused, offset=offset)
    out, bound = c.ref()
    lg = c.logits64()[:, c.H:c.H + c.T]
    sd = float(lg.std())
    assert 3.0 <= sd <= 5.0, sd
    if fused:  # exact float32 logits
        assert E.lattice(c.a1, c.wc) >= 0.25 and float((c.a1.double().abs() @ c.wc.double().abs().T).max()) * 8 < 2 ** 24
    step = G.bf16_step(out)
    print("fused %s offset %g: logit sd %.2f, median bound / bf16 step %.3f, max %.3f" % (
        fused, offset, sd, float((bound / step).median()), float((bound / step).max())))
    if offset == 0.0:
        assert float((bound / step).median()) < 0.5
    w = E.asp_weights(lg).float()
    x = c.x[:, c.H:c.H + c.T].float()
    s0, s1, s2 = w.sum(1), (w * x).sum(1), (w * x * x).sum(1)
    mean = s1 / s0
    sdv = (s2 / s0 - mean * mean).clamp(min=1e-12).sqrt()
    emu = torch.cat([mean * c.sc[:c.C] + c.sh[:c.C], sdv * c.sc[c.C:] + c.sh[c.C:]], 1)
    assert bool(((emu.double() - out).abs() <= bound).all())
    assert bool(E.in_interval(emu.bfloat16(), out, bound).all())


# ---- time mean, apply, add, pack ---------------------------------------------------------------------------------------------------------
def test_small_kernel_cases():
    for T in E.MEAN_TS:
        x, ref, bound = E.mean_case(2, T, 64)
        assert T * 20 < 2 ** 24 and bool((x[:, :2] == E.POISON).all())
        assert bool((bound == 0).all()) == (T & (T - 1) == 0)
        wrong = x[:, 2:2 + T].double().sum(1) / (T + 4)      # mean over T + 2 H rows
        if T > 1:
            assert not bool(E.in_interval(wrong.float().bfloat16(), ref, bound).all())
        assert E.multi_share(ref, bound) <= 0.02
    x, gate, res, want = E.apply_case(2, 5, 64)
    exact = x[:, 2:7].double() * gate.double()[:, None] + res[:, 2:7].double()
    assert E.lattice(exact) >= 2.0 ** -8 and float(exact.abs().max()) < 2 ** 15        # exact in float32
    assert float((E.rne(exact) != exact).double().mean()) >= 0.05                      # really rounded
    assert not torch.equal(E.trunc(exact).bfloat16(), want[:, 2:7])
    a, b, w = E.add_case(5, 24)
    s = a.float() + b.float()
    assert int(G.is_tie(s[0, :8]).sum()) >= 6 and not torch.equal(G.truncate_bf16(s), w)
    assert float(w[0, 0]) == 256.0 and float(w[0, 1]) == 260.0                         # ties to even, below an even and an odd neighbour
    xp = E.pack_case(2, 3, 17)
    assert int(G.is_tie(xp[:, 0, :7]).sum()) == 2 * 5
    wp = E.pack_ref(xp, 2, 24)
    assert float(wp[0, 2, 0]) == 1.0 and float(wp[0, 2, 1]) == 1.0 + 2.0 ** -6 and bool((wp[:, :, 17:] == 0).all()) and bool((wp[:, :2] == 0).all())


# ---- SE --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (512, 1024))
@pytest.mark.parametrize("S", sorted(set(E.SE_GATE_S) | {16, 48}))
def test_se_case_conditions(C, S):
    c = E.SeCase(C, S)
    assert c.margin() < 1
    h = c.hidden(c.mean.double())
    assert torch.equal(h, h.round()) and len(set(h[0].tolist())) >= 3 and not torch.equal(h[0], h[1])
    y = c.pre()
    assert torch.equal(y[0], c.target.double())
    assert float((y.abs() <= 8).double().mean()) >= 0.5
    lo, hi = c.gate_interval()
    share = float((lo != hi).double().mean())
    print("C %d S %d: gate intervals with two values %.4f, |y| <= %.1f" % (C, S, share, float(y.abs().max())))
    assert share <= 0.02
    assert bool(((hi.double() - lo.double()).abs() <= G.bf16_step(hi.double())).all())  # at most adjacent
    assert float(y.abs().max()) < 60  # x g + res stays a float32-exact sum only while g is not tiny; the reference rounds like the device anyway


@pytest.mark.parametrize("defect", E.SE_DEFECTS)
def test_se_defects_are_rejected(defect):
    C, S, T = (512, 48, 300)
    c = E.SeCase(C, S if defect != "w1_row_reuse" else 24, T=T)
    H = c.H
    lo, hi = c.gate_interval()
    good = torch.sigmoid(c.pre()).float().bfloat16()
    assert bool(((good >= lo) & (good <= hi)).all()) and bool(E.block_matches(c.block_ref(good), c, lo, hi).all())

    def gate_rejected(g):
        return not bool(((g >= lo) & (g <= hi)).all())

    if defect == "mean_T2H":
        m = E.rne(c.mean.double() * T / (T + 2 * H))
        g = torch.sigmoid(c.pre(mean=m)).float().bfloat16()
        assert gate_rejected(g) and not bool(E.block_matches(c.block_ref(g), c, lo, hi).all())
    elif defect == "gate_xor1":
        for site in (0, 101, C - 1):
            g = good.clone()
            g[:, site] = good[:, site ^ 1]
            assert gate_rejected(g) and not bool(E.block_matches(c.block_ref(g), c, lo, hi).all()), site
    elif defect == "w1_row_reuse":
        moved = 0
        for wave in range(8):  # (two rows of W1 can meet the same two means in the same sum: then there is nothing to see)
            if torch.equal(c.hidden(c.mean.double(), defect, wave), c.hidden(c.mean.double())):
                continue
            moved += 1
            g = torch.sigmoid(c.pre(defect=defect, site=wave)).float().bfloat16()
            assert gate_rejected(g), wave
        assert moved >= 7
    else:
        got = c.block_ref(good)
        rows = [H + 256] if defect == "skip_256" else list(range(H)) + list(range(H + T, T + 2 * H))
        G._bits(got)[:, rows] = G.BF16_CANARY
        assert not bool(E.block_matches(got, c, lo, hi).all())
        assert _window_with(c.block_ref(good).view(-1, C), got.view(-1, C)) is not None


@pytest.mark.parametrize("defect", ("gate_xor1", "w1_row_reuse"))
def test_se_defects_the_old_tolerance_accepts(defect):
    """(+) on random operands drawn like the old gate test's at its batch of 1 (S = 24 for the row reuse, which that test never ran):
    a pair of channels whose gates differ by less than 5e-3; a wave whose last two hidden units move no gate by 5e-3."""
    C, S, b = 512, (24 if defect == "w1_row_reuse" else 128), 1
    g = torch.Generator().manual_seed(C + S)
    mean = torch.randn(b, C, generator=g).bfloat16().double()
    w1, b1 = (torch.randn(S, C, generator=g) / 16).bfloat16().double(), (torch.randn(S, generator=g) * 0.2).double()
    w2, b2 = (torch.randn(C, S, generator=g) / 8).bfloat16().double(), (torch.randn(C, generator=g) * 0.2).double()

    def gates(w1_):
        return torch.sigmoid(torch.relu(mean @ w1_.T + b1) @ w2.T + b2)

    want = gates(w1)
    accepted = 0
    if defect == "gate_xor1":
        for site in range(C):
            got = want.clone()
            got[:, site] = want[:, site ^ 1]
            accepted += E.gate_old_check(got.float().bfloat16(), want)
    else:
        rows = S // 8
        for wave in range(8):
            w = w1.clone()
            w[wave * rows + rows - 1] = w1[wave * rows + rows - 2]
            accepted += E.gate_old_check(gates(w).float().bfloat16(), want)
    print(defect, "accepted at", accepted, "sites")
    assert accepted >= 1


# ---- Linear ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_cases_and_defects(shape):
    M, N, K = shape
    c = G.Case(M, N, K, seed=9)
    assert G.exact_bound(K) < 2 ** 23
    want = E.linear_ref(c)
    assert torch.equal(want, (G.z_int64(c.a, c.w) + c.bias.long()).double())
    for bias in (True, False):
        ref = E.linear_ref(c, bias).float()
        win = G.Window(M, N, torch.float32, "a8").snapshot()
        win.view.copy_(ref)
        assert G.check_window(win, ref, (16, 16)) is None
        for wave in range(8):
            win.view.copy_(E.linear_ref(c, bias, "slice_dropped", wave).float())
            assert G.check_window(win, ref, (16, 16)) is not None
    win.view.copy_(E.linear_ref(c, True, "bias_n0").float())
    assert G.check_window(win, E.linear_ref(c).float(), (16, 16)) is not None
    ks = E.linear_hot_ks(K)
    kw = K // 8
    assert sorted(set(ks)) == sorted(ks) and all(w * kw in ks and (w + 1) * kw - 1 in ks for w in range(8))
    a, w, awant, kk = E.linear_address_case(N, K)
    assert a.shape[0] % 16 == 0 and torch.equal(a.double() @ w.double().T, awant.double())
    for wave in range(8):  # a dropped slice empties the rows whose hot k it holds
        a2 = a.clone()
        a2[:, wave * kw:(wave + 1) * kw] = 0
        assert not torch.equal(a2.double() @ w.double().T, awant.double())
