"""GPU: every non-GEMM launch of csrc/ecapa_kernels.hip and csrc/res2net_fused.hip through the C ABI against the exact references
of tests/ecapa_cases.py (constructions, conditions and the derivation of the bounds: its docstring; test_ecapa_cases_cpu.py asserts
the conditions and shows that the comparators used here reject the defects these kernels could have).

Every output sits in a gemm_cases.Window: canary rows above and below, canary columns wherever the entry point takes a leading
dimension.  Every input is copied before the launch and compared bit for bit after it; halo rows and pad columns of the inputs hold
poison.  Layouts are the ones the launchers accept; the refusals are a table of their own and launch nothing.

Measured on an MI355X (test_asp_bounded and test_se_gate print them on every run, pytest -s).  The bounded ASP cases use the DERIVED
per-element bound of ecapa_cases.asp_bound, not the 2 S rule (which is asserted beside it on the relative rms error):
    entry point / kernel, (B, T, C), offset on x     max |err| / bound      two-valued intervals    outputs = nearest bf16
    ma_asp_fused_bf16   (2, 130, 256)   0                  0.0000                 17.1 %                  100 %
    ma_asp_fused_bf16   (2, 300, 512)   0                  0.0000                 17.4 %                  100 %
    ma_asp_fused_bf16   (2, 130, 256)   16                 0.0006                 52.1 %                  98.6 %
    asp_pool8_kernel    (2, 130, 192)   0                  0.0000                 16.2 %                  100 %
    asp_pool8_kernel    (2, 130, 192)   16                 0.0006                 51.7 %                  97.9 %
    asp_pool_kernel     (2, 70, 72)     0                  0.0000                 17.0 %                  100 %
    asp_pool_kernel     (2, 70, 72)     16                 0.0006                 51.0 %                  97.9 %
The ratio is 0 where every output is the bf16 number nearest to the float64 value; the worst-case bound (every rounding of T terms
and eight chained exponentials aligned) is about a thousand times what the hardware does, and with mean^2 = 256 var the cancellation
of S2 / S0 - mean^2 is what the 0.0006 and the 2 % of outputs one bf16 step off show.  Relative rms error over that of rounding
the exact result to bf16 (must be <= 2): 1.000 on all seven.  Selector cases: at most 2 % of a case's
outputs have an interval of two bf16 numbers (asserted on the CPU), the mean half none.  SE: no gate interval of the gate and block
cases holds two values (0.0 % on all ten (C, S) of test_se_gate), so se_block is held to one gate per (utterance, channel) and is
bit-equal to the three separate launches on every case.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecapa_cases as E  # noqa: E402
import gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
INV, UNS = -1, -5


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _lib

    assert torch.cuda.is_available()
    return _lib.load()


def _stream():
    from mindaudio_amd import _host

    return _host.current_stream_ptr()


class Inputs:
    """Device copies of the inputs of one launch, each inside a wider poison-filled buffer when it has a leading dimension."""

    def __init__(self):
        self.items = []

    def add(self, t, ld=None, fill=E.POISON):
        t = t.to(DEV)
        if ld is None:
            buf = view = t.contiguous()
        else:
            buf, view = E.embed(t, ld, fill)
        self.items.append((buf, buf.clone()))
        return view

    def check(self):
        torch.cuda.synchronize()
        for buf, snap in self.items:
            assert torch.equal(G._bits(buf) if buf.dtype in (F32, BF16) else buf, G._bits(snap) if snap.dtype in (F32, BF16) else snap), "an input was written"


def _ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def _guard(win):
    """The guard band alone (the window's content is judged by the caller): every element inside must have been written."""
    return G.check_window(win, win.view.clone(), (16, 32))


# ---- Res2Net ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", E.R2_CCS)
@pytest.mark.parametrize("shape", E.R2_SHAPES, ids=lambda s: "T%d_H%d_d%d" % s)
def test_res2net_chain_bit_exact(lib, cc, shape):
    """All tp rows and 8 cc columns of y equal the float64 chain with the kernel's rounding points: zero halo rows in steps 1 .. 7,
    y_0 = x_0 on all rows, ldx != ldy, three distinct utterances."""
    T, H, d = shape
    c = E.Res2Case(cc, T, H, d, seed=T + cc)
    want = c.ref().view(-1, c.C).bfloat16().to(DEV)
    ins = Inputs()
    x = ins.add(c.x.view(-1, c.C), ld=c.C + 8)
    w, bias, sc, sh = ins.add(c.w), ins.add(c.bias), ins.add(c.scale), ins.add(c.shift)
    win = G.Window(c.B * c.tp, c.C, BF16, "a8", DEV).snapshot()
    assert win.ld != x.stride(0) and win.ld > c.C and x.stride(0) > c.C
    _ok(lib.ma_res2net_fused_bf16(x.data_ptr(), x.stride(0), win.view.data_ptr(), win.ld, c.B, T, H, cc, 8, d, w.data_ptr(), bias.data_ptr(),
                                  sc.data_ptr(), sh.data_ptr(), _stream()))
    msg = G.check_window(win, want, (16, 32))
    assert msg is None, "cc %d T %d H %d d %d: %s (row = utterance * %d + frame row, column = step * %d + channel)" % (cc, T, H, d, msg, c.tp, cc)
    ins.check()


# ---- ASP: selector cases ------------------------------------------------------------------------------------------------------------------
def _asp_fused(lib, c, ins):
    a1 = ins.add(c.a1.view(-1, 128), ld=136, fill=1.0)
    x = ins.add(c.x.view(-1, c.C), ld=c.C + 8)
    wc, sc, sh = ins.add(c.wc), ins.add(c.sc), ins.add(c.sh)
    win = G.Window(c.B, 2 * c.C, BF16, "tight", DEV).snapshot()
    _ok(lib.ma_asp_fused_bf16(a1.data_ptr(), a1.stride(0), wc.data_ptr(), x.data_ptr(), x.stride(0), c.B, c.T, c.H, c.C, 128, E.EPS,
                              sc.data_ptr(), sh.data_ptr(), win.view.data_ptr(), _stream()))
    return win


def _asp_pool(lib, c, ins, ldl, ldx):
    lg = ins.add(c.logits.view(-1, c.C), ld=ldl, fill=0.0)
    x = ins.add(c.x.view(-1, c.C), ld=ldx)
    sc, sh = ins.add(c.sc), ins.add(c.sh)
    win = G.Window(c.B, 2 * c.C, BF16, "tight", DEV).snapshot()
    _ok(lib.ma_asp_pool_bf16(lg.data_ptr(), lg.stride(0), x.data_ptr(), x.stride(0), c.B, c.T, c.H, c.C, E.EPS, sc.data_ptr(),
                             sh.data_ptr(), win.view.data_ptr(), _stream()))
    return win


def _check_selector(c, win, what):
    out, parts = c.ref()
    lo, hi = E.bf16_interval(out, E.std_bound(out, parts))
    msg = G.check_window(win, None, (1, 16), lo=lo.to(DEV), hi=hi.to(DEV))
    assert msg is None, "%s (B, T, C) = (%d, %d, %d): %s (columns < C: mean, >= C: std)" % (what, c.B, c.T, c.C, msg)
    # the mean half is exact: one admissible value
    assert torch.equal(win.view[:, :c.C].cpu(), out[:, :c.C].float().bfloat16())


@pytest.mark.parametrize("shape", E.ASP_FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_asp_fused_selector(lib, shape):
    c = E.AspCase(*shape, fused=True)
    ins = Inputs()
    win = _asp_fused(lib, c, ins)
    _check_selector(c, win, "asp_fused")
    ins.check()


@pytest.mark.parametrize("shape", E.ASP_POOL8_SHAPES + E.ASP_SCALAR_SHAPES + [(2, 33, 64, "ldl"), (2, 70, 64, "ldl")],
                         ids=lambda s: "x".join(map(str, s)))
def test_asp_pool_selector(lib, shape):
    """asp_pool8_kernel (C % 64 == 0, 16-byte rows) and the scalar asp_pool_kernel (C = 72, C = 40, or ldl % 8 != 0)."""
    B, T, C = shape[:3]
    c = E.AspCase(B, T, C, fused=False)
    ldl = C + 4 if len(shape) == 4 else C + 8
    ins = Inputs()
    win = _asp_pool(lib, c, ins, ldl, C + 16)
    _check_selector(c, win, "asp_pool")
    ins.check()


# ---- ASP: bounded cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,offset", [("fused", (2, 130, 256), 0.0), ("fused", (2, 300, 512), 0.0), ("fused", (2, 130, 256), 16.0),
                                                 ("pool8", (2, 130, 192), 0.0), ("pool8", (2, 130, 192), 16.0), ("scalar", (2, 70, 72), 0.0),
                                                 ("scalar", (2, 70, 72), 16.0)])
def test_asp_bounded(lib, kernel, shape, offset):
    """Random bf16 operands, logits of standard deviation 4 (offset 16 on x: mean^2 >> var), against float64 on the same operands within
    the DERIVED per-element bound of ecapa_cases.asp_bound (not the 2 S rule)."""
    c = E.AspRandomCase(*shape, fused=(kernel == "fused"), offset=offset)
    ins = Inputs()
    win = _asp_fused(lib, c, ins) if kernel == "fused" else _asp_pool(lib, c, ins, c.C + 8, c.C + 16)
    out, bound = c.ref()
    got = win.view.cpu()
    ratio = E.preimage_ratio(got, out, bound)
    print("asp %s %s offset %g: max |err| / bound %.4f (mean half %.4f, std half %.4f), intervals of two values %.4f, nearest bf16 %.4f" % (
        kernel, shape, offset, ratio, E.preimage_ratio(got[:, :c.C], out[:, :c.C], bound[:, :c.C]),
        E.preimage_ratio(got[:, c.C:], out[:, c.C:], bound[:, c.C:]), E.multi_share(out, bound), E.nearest_share(got, out)))
    lo, hi = E.bf16_interval(out, bound)
    msg = G.check_window(win, None, (1, 16), lo=lo.to(DEV), hi=hi.to(DEV))
    assert msg is None, msg
    assert ratio <= 1
    # beside the per-element bound, the project's aggregate rule: relative rms error <= 2 S, S = that of rounding the exact result to bf16
    e, S = E.relrms(got.double(), out), E.relrms(out.float().bfloat16().double(), out)
    print("    relative rms error %.3e, rounding-only %.3e, ratio %.3f" % (e, S, e / S))
    assert e <= 2 * S
    ins.check()


# ---- time mean, apply, add, pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", E.MEAN_LAYOUTS, ids=lambda v: "C%d_ld%d_%s" % v)
def test_time_mean(lib, layout):
    """time_mean8_kernel (C % 64 == 0, ldx % 8 == 0) and the scalar time_mean_kernel (C = 72; C = 64 with ldx % 8 != 0): bit equal when T
    is a power of two, else within the interval of the one division."""
    C, ldx, _ = layout
    for T in E.MEAN_TS:
        x, ref, bound = E.mean_case(2, T, C)
        ins = Inputs()
        xd = ins.add(x.view(-1, C), ld=ldx)
        win = G.Window(2, C, BF16, "tight", DEV).snapshot()
        _ok(lib.ma_time_mean_bf16(xd.data_ptr(), ldx, 2, T, 2, C, win.view.data_ptr(), _stream()))
        lo, hi = E.bf16_interval(ref, bound)
        msg = G.check_window(win, None, (1, 64), lo=lo.to(DEV), hi=hi.to(DEV))
        assert msg is None, "T %d: %s" % (T, msg)
        if T & (T - 1) == 0:
            assert torch.equal(win.view.cpu(), ref.float().bfloat16())
        ins.check()


@pytest.mark.parametrize("T,C", [(5, 64), (33, 512), (1, 8)])
def test_se_apply(lib, T, C):
    x, gate, res, want = E.apply_case(2, T, C)
    ins = Inputs()
    xd, rd, gd = ins.add(x.view(-1, C), ld=C + 8), ins.add(res.view(-1, C), ld=C + 24), ins.add(gate)
    win = G.Window(2 * (T + 4), C, BF16, "a8", DEV).snapshot()
    assert len({xd.stride(0), rd.stride(0), win.ld}) == 3
    _ok(lib.ma_se_apply_bf16(xd.data_ptr(), xd.stride(0), gd.data_ptr(), rd.data_ptr(), rd.stride(0), win.view.data_ptr(), win.ld, 2, T, 2, C,
                             _stream()))
    msg = G.check_window(win, want.view(-1, C).to(DEV), (T + 4, 8))
    assert msg is None, msg
    ins.check()


@pytest.mark.parametrize("cols", (8, 24, 520))
def test_add(lib, cols):
    """IEEE float32 add, then round to nearest even (hand-built ties in row 0); b == NULL copies."""
    rows = 37
    a, b, want = E.add_case(rows, cols)
    ins = Inputs()
    ad, bd = ins.add(a, ld=cols + 8), ins.add(b, ld=cols + 24)
    for second in (bd, None):
        win = G.Window(rows, cols, BF16, "a8", DEV).snapshot()
        assert len({ad.stride(0), bd.stride(0), win.ld}) == 3
        _ok(lib.ma_add_bf16(ad.data_ptr(), ad.stride(0), second.data_ptr() if second is not None else None, bd.stride(0) if second is not None else 0,
                            win.view.data_ptr(), win.ld, rows, cols, _stream()))
        msg = G.check_window(win, (want if second is not None else a).to(DEV), (rows, 8))
        assert msg is None, msg
    ins.check()


@pytest.mark.parametrize("B,T,F,H,Cpad", [(2, 5, 80, 4, 96), (2, 7, 17, 2, 24), (3, 7300, 80, 4, 96)])
def test_pack_input(lib, B, T, F, H, Cpad):
    """float32 -> bf16 with ties to even and to odd neighbours, zero halo rows and pad channels; the last case has more elements than
    the grid cap of 8192 x 256 threads."""
    if T > 1000:
        assert B * (T + 2 * H) * Cpad > 8192 * 256
    x = E.pack_case(B, T, F)
    ins = Inputs()
    xd = ins.add(x)
    win = G.Window(B * (T + 2 * H), Cpad, BF16, "tight", DEV).snapshot()
    _ok(lib.ma_ecapa_pack_input_bf16(xd.data_ptr(), B, T, F, H, Cpad, win.view.data_ptr(), _stream()))
    msg = G.check_window(win, E.pack_ref(x, H, Cpad).view(-1, Cpad).to(DEV), (T + 2 * H, Cpad))
    assert msg is None, msg
    ins.check()


# ---- SE ----------------------------------------------------------------------------------------------------------------------------------
def _se_weights(c, ins):
    return [ins.add(v).data_ptr() for v in (c.w1, c.b1, c.w2, c.b2)]


@pytest.mark.parametrize("C", (512, 1024))
@pytest.mark.parametrize("S", E.SE_GATE_S)
def test_se_gate(lib, C, S):
    c = E.SeCase(C, S)
    ins = Inputs()
    mean = ins.add(c.mean)
    w1, b1, w2, b2 = _se_weights(c, ins)
    win = G.Window(c.B, C, BF16, "tight", DEV).snapshot()
    _ok(lib.ma_se_gate_bf16(mean.data_ptr(), w1, b1, w2, b2, win.view.data_ptr(), c.B, C, S, _stream()))
    lo, hi = c.gate_interval()
    msg = G.check_window(win, None, (1, 64), lo=lo.to(DEV), hi=hi.to(DEV))
    assert msg is None, "C %d S %d: %s" % (C, S, msg)
    print("se_gate C %d S %d: gate intervals of two values %.4f" % (C, S, float((lo != hi).double().mean())))
    ins.check()


@pytest.mark.parametrize("C,S,T", E.SE_BLOCK, ids=lambda v: str(v))
def test_se_block(lib, C, S, T):
    """out[t, c] = bf16(x g + res) for ONE admissible gate g per (b, c) on all T frames, zero halo rows, canaries elsewhere; and the
    whole buffer equals, bit for bit, what ma_time_mean_bf16 + ma_se_gate_bf16 + ma_se_apply_bf16 leave (the only inexact quantity,
    the sigmoid, is the same expression on the same exact argument).  Where a gate interval holds two values the interval decides."""
    c = E.SeCase(C, S, T=T)
    H, B, tp = c.H, c.B, T + 2 * c.H
    ins = Inputs()
    x, res = ins.add(c.x.view(-1, C), ld=C + 8), ins.add(c.res.view(-1, C), ld=C + 24)
    w1, b1, w2, b2 = _se_weights(c, ins)
    win = G.Window(B * tp, C, BF16, "a8", DEV).snapshot()
    assert len({x.stride(0), res.stride(0), win.ld}) == 3 and min(x.stride(0), res.stride(0), win.ld) > C
    _ok(lib.ma_se_block_bf16(x.data_ptr(), x.stride(0), w1, b1, w2, b2, res.data_ptr(), res.stride(0), win.view.data_ptr(), win.ld, B, T, H, C, S,
                             _stream()))
    msg = _guard(win)
    assert msg is None, msg
    lo, hi = c.gate_interval()
    got = win.view.cpu().view(B, tp, C)
    ok = E.block_matches(got, c, lo, hi)
    assert bool(ok.all()), "C %d S %d T %d: %d (utterance, channel) pairs match no admissible gate, first %s" % (
        C, S, T, int((~ok).sum()), (~ok).nonzero()[0].tolist())
    # the three launches
    mean = G.Window(B, C, BF16, "tight", DEV).snapshot()
    gate = G.Window(B, C, BF16, "tight", DEV).snapshot()
    win3 = G.Window(B * tp, C, BF16, "a8", DEV).snapshot()
    _ok(lib.ma_time_mean_bf16(x.data_ptr(), x.stride(0), B, T, H, C, mean.view.data_ptr(), _stream()))
    assert G.check_window(mean, c.mean.to(DEV), (1, 64)) is None
    _ok(lib.ma_se_gate_bf16(mean.view.data_ptr(), w1, b1, w2, b2, gate.view.data_ptr(), B, C, S, _stream()))
    assert G.check_window(gate, None, (1, 64), lo=lo.to(DEV), hi=hi.to(DEV)) is None
    _ok(lib.ma_se_apply_bf16(x.data_ptr(), x.stride(0), gate.view.data_ptr(), res.data_ptr(), res.stride(0), win3.view.data_ptr(), win3.ld, B, T, H,
                             C, _stream()))
    assert torch.equal(G._bits(win.buf), G._bits(win3.buf)), "se_block differs from time_mean + se_gate + se_apply"
    assert torch.equal(got, c.block_ref(gate.view.cpu()))
    ins.check()


# ---- the embedding Linear -----------------------------------------------------------------------------------------------------------------
def _linear(lib, a, w, bias, win, K):
    M, N = win.M, win.N
    _ok(lib.ma_linear_small_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr() if bias is not None else None,
                                 win.view.data_ptr(), win.ld, M, N, K, _stream()))


@pytest.mark.parametrize("shape", E.LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_small(lib, shape):
    """Integer-exact products (float32 output bit equal, lda, ldw > K, ldo > N, with and without bias) and the address case whose hot
    k's are the first and last column of every wave's K slice and of every 384-column block."""
    M, N, K = shape
    c = G.Case(M, N, K, seed=9)
    ins = Inputs()
    a, w, bias = ins.add(c.a, ld=K + 8, fill=2.0), ins.add(c.w, ld=K + 16, fill=2.0), ins.add(c.bias)
    for with_bias in (True, False):
        win = G.Window(M, N, F32, "a8", DEV).snapshot()
        assert win.ld > N
        _linear(lib, a, w, bias if with_bias else None, win, K)
        msg = G.check_window(win, E.linear_ref(c, with_bias).float().to(DEV), (16, 16))
        assert msg is None, "bias %s: %s" % (with_bias, msg)
    aa, ww, want, ks = E.linear_address_case(N, K)
    a2, w2 = ins.add(aa, ld=K + 8, fill=1.0), ins.add(ww, ld=K + 16, fill=1.0)
    Ma = aa.shape[0]
    for with_bias in (True, False):
        win = G.Window(Ma, N, F32, "a8", DEV).snapshot()
        _linear(lib, a2, w2, bias if with_bias else None, win, K)
        ref = want + (c.bias[None, :] if with_bias else 0.0)
        msg = G.check_window(win, ref.to(DEV), (16, 16),
                             explain=lambda r, col, got: "row %d is hot at k = %d (wave %d, column %d of its slice)" % (
                                 r, int(ks[r]), int(ks[r]) // (K // 8), int(ks[r]) % (K // 8)))
        assert msg is None, "address case, bias %s: %s" % (with_bias, msg)
    ins.check()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def refusal_table(P, Q, O, LD):
    """Every MA_ERR_INVALID_ARG / MA_ERR_UNSUPPORTED condition of the launchers of the two files as (entry point, what was changed,
    arguments, expected code).  P, Q: 16-byte aligned input pointers, O: the output pointer, LD its leading dimension (>= 1024,
    % 8 == 0).  The unchanged arguments are consistent with buffers of 1 MiB."""
    rows = []

    def entry(fn, names, good, muts):
        for mut, code in muts:
            a = dict(zip(names, good))
            a.update(mut)
            rows.append((fn, ", ".join("%s=%s" % kv for kv in mut.items()), [a[n] for n in names], code))

    def nulls(*names):
        return [({n: None}, INV) for n in names]

    def off2(*pairs):
        return [({n: p + 2}, UNS) for n, p in pairs]

    entry("ma_ecapa_pack_input_bf16", "x batch T F halo Cpad out stream".split(), [P, 2, 5, 17, 2, 24, O, None],
          nulls("x", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"F": 0}, INV), ({"halo": -1}, INV), ({"Cpad": 16}, INV)])
    entry("ma_add_bf16", "a lda b ldb out ldo rows cols stream".split(), [P, 32, Q, 40, O, LD, 4, 16, None],
          nulls("a", "out") + [({"rows": 0}, INV), ({"cols": 7}, INV), ({"cols": 0}, INV), ({"cols": 12}, UNS), ({"lda": 33}, UNS),
                               ({"ldo": LD + 1}, UNS), ({"ldb": 41}, UNS)])
    entry("ma_time_mean_bf16", "x ldx batch T halo C out stream".split(), [P, 64, 2, 5, 2, 64, O, None],
          nulls("x", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"C": 0}, INV), ({"batch": 65536}, INV)])
    entry("ma_se_apply_bf16", "x ldx gate residual ldr out ldo batch T halo C stream".split(), [P, 72, Q, P, 80, O, LD, 2, 5, 2, 64, None],
          nulls("x", "gate", "residual", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"C": 4}, INV), ({"C": 12}, UNS),
                                                   ({"ldx": 73}, UNS), ({"ldr": 81}, UNS), ({"ldo": LD + 1}, UNS)])
    entry("ma_asp_pool_bf16", "logits ldl x ldx batch T halo C eps sc sh out stream".split(), [P, 72, Q, 72, 2, 5, 2, 64, E.EPS, P, Q, O, None],
          nulls("logits", "x", "sc", "sh", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"C": 0}, INV),
                                                     ({"batch": 65536}, INV)])
    entry("ma_asp_fused_bf16", "a1 lda Wc x ldx batch T halo C att eps sc sh out stream".split(),
          [P, 136, Q, P, 264, 2, 5, 2, 256, 128, E.EPS, P, Q, O, None],
          nulls("a1", "Wc", "x", "sc", "sh", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"C": 0}, INV),
                                                       ({"batch": 65536}, INV), ({"att": 64}, UNS), ({"C": 128}, UNS), ({"lda": 137}, UNS),
                                                       ({"ldx": 265}, UNS), ({"lda": 120}, UNS), ({"ldx": 248}, UNS)]
          + off2(("a1", P), ("Wc", Q), ("x", P), ("out", O)))
    entry("ma_se_gate_bf16", "mean W1 b1 W2 b2 gate batch C S stream".split(), [P, Q, P, Q, P, O, 2, 512, 64, None],
          nulls("mean", "W1", "b1", "W2", "b2", "gate") + [({"batch": 0}, INV), ({"C": 0}, INV), ({"S": 0}, INV), ({"C": 256}, UNS),
                                                           ({"S": 12}, UNS), ({"S": 136}, UNS)] + off2(("mean", P), ("W1", Q), ("W2", Q)))
    entry("ma_linear_small_bf16", "a lda W ldw bias out ldo M N K stream".split(), [P, 3080, Q, 3088, P, O, LD, 16, 16, 3072, None],
          nulls("a", "W", "out") + [({"M": 0}, INV), ({"N": 0}, INV), ({"K": 0}, INV), ({"M": 8}, UNS), ({"N": 8}, UNS), ({"K": 3000}, UNS),
                                    ({"lda": 3081}, UNS), ({"ldw": 3089}, UNS), ({"lda": 3064}, UNS), ({"ldw": 3064}, UNS), ({"ldo": 8}, UNS),
                                    ({"M": 16 * 65536}, UNS)] + off2(("a", P), ("W", Q)))
    entry("ma_se_block_bf16", "x ldx W1 b1 W2 b2 residual ldr out ldo batch T halo C S stream".split(),
          [P, 520, Q, P, Q, P, P, 536, O, LD, 2, 5, 2, 512, 64, None],
          nulls("x", "W1", "b1", "W2", "b2", "residual", "out") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"batch": 2 ** 31}, INV),
                                                                   ({"C": 256}, UNS), ({"S": 24}, UNS), ({"S": 144}, UNS), ({"S": 0}, UNS),
                                                                   ({"ldx": 521}, UNS), ({"ldr": 537}, UNS), ({"ldo": LD + 1}, UNS),
                                                                   ({"ldx": 504}, UNS), ({"ldr": 504}, UNS), ({"ldo": 504}, UNS)]
          + off2(("x", P), ("W1", Q), ("W2", Q), ("residual", P), ("out", O)))
    entry("ma_res2net_fused_bf16", "x ldx y ldy batch T halo cc scale dil w bias sc sh stream".split(),
          [P, 520, O, LD, 2, 5, 4, 64, 8, 2, Q, P, Q, P, None],
          nulls("x", "y", "w", "bias", "sc", "sh") + [({"batch": 0}, INV), ({"T": 0}, INV), ({"halo": -1}, INV), ({"scale": 1}, INV), ({"dil": 0}, INV),
                                                      ({"cc": 32}, UNS), ({"dil": 5}, UNS), ({"T": 400}, UNS), ({"ldx": 521}, UNS),
                                                      ({"ldy": LD + 1}, UNS), ({"ldx": 504}, UNS), ({"ldy": 504}, UNS), ({"scale": 4}, UNS),
                                                      ({"cc": 128, "ldx": 1032, "halo": 100, "T": 184, "dil": 90}, UNS)]  # the tile outgrows the LDS
          + off2(("x", P), ("y", O), ("w", Q)))  # 16-byte loads and stores
    return rows


def test_refusals(lib):
    """Nothing is launched: the code comes back and the output window is untouched."""
    scratch = torch.zeros(2, 1 << 18, dtype=torch.int16, device=DEV)  # two inputs of 512 KiB
    win = G.Window(64, 1024, BF16, "a8", DEV).snapshot()
    rows = refusal_table(scratch[0].data_ptr(), scratch[1].data_ptr(), win.view.data_ptr(), win.ld)
    assert len({r[0] for r in rows}) == 10
    for fn, what, args, code in rows:
        rc = getattr(lib, fn)(*args)
        assert rc == code, "%s(%s) returned %d, not %d" % (fn, what, rc, code)
    torch.cuda.synchronize()
    assert torch.equal(G._bits(win.buf), win.before) and not bool(scratch.any())
