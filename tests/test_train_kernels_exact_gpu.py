"""Element-wise, guard-banded GPU tests of the memory-bound training-step kernels (mindaudio_amd/csrc/train_kernels.hip) against the
float64 references, restated dropout mask, derived bounds and comparators of tests/train_kernel_cases.py (whose CPU self-test shows
that a float32 restatement passes every check used here and that every planted defect fails it).

Every output lives in a window of a sentinel-filled buffer (NaN 0x7FC0BEEF for float32, 0xABCD for bf16) with guard rows in front of
and behind it and, where the entry point takes a row stride, guard columns: the guards must come back untouched and every element the
operation owns must have been written.  Dropout sites are compared with the restated mask BIT FOR BIT (out != 0 reads the mask:
inputs are bounded away from zero) at the index the site documents, kept values are the undropped result times inv_keep.

Worst error / bound measured on an MI355X (exact: bit for bit, no figure):
  Swish sites (the ReLU sites, dropout_add, dropout_bwd and dy_next are exact).  A bf16 output is held to the bf16 roundings of the
  two ends of its float32 interval, which are one bf16 step apart where the interval straddles a rounding boundary: 1 = an end:
    act_dropout swish bf16 fwd                           1
    act_dropout swish bf16 bwd                           1
    act_dropout swish x32 fwd                            0.333
    act_dropout swish x32 bwd                            0.333
  GEMM-epilogue sites, m = 70 (integer products; the saturated Swish intervals collapse to one bf16 value: all bit for bit):
    dense_act_drop / dense_act_drop_bwd, Swish and ReLU, n = 512          0
    dense_join k = 256 (gemm_k256) and k = 512 (rows_packed)               exact
    ffn_train hidden = 256: h, the gk tape; x_out from the stored h        0, exact
  layernorm_bwd (g, dgamma, dbeta; worst over dy float32 / bf16, accumulate on / off, dgamma= / partials=), D = 256 / 512 / 768 / 1024:
    rows 1                                               0.345 / 0.69 / 0.464 / 0.716
    rows 3                                               0.14 / 0.113 / 0.12 / 0.0979
    rows 5                                               0.186 / 0.113 / 0.129 / 0.131
    rows 4099                                            0.369 / 0.355 / 0.286 / 0.255
    in place                                             0.106 / 0.0936 / 0.121 / 0.0983
    one-hot row 0                                        0.104 / 0.0766 / 0.115 / 0.0777
    one-hot row 4098                                     0.109 / 0.131 / 0.0961 / 0.0783
    one-hot row 4097                                     0.0879 / 0.0865 / 0.0917 / 0.0797
  layernorm_bwd_next rows 5 (g, dgamma, dbeta; dy_next exact) 0.186
  layernorm_bwd_next rows 4099 (g, dgamma, dbeta; dy_next exact) 0.407
  bn_finalize C 16 (nparts 1/15/16/17/112/113/128/129/300, count = 1) 0.373
  bn_finalize C 24 (nparts 1/15/16/17/112/113/128/129/300, count = 1) 0.46
  bn_finalize C 256 (nparts 1/15/16/17/112/113/128/129/300, count = 1) 0.491
  convmid_fwd_train ks 3 z                               0.439
  convmid_fwd_train ks 3 sum z | sum z^2                 0.0901
  convmid_fwd_train_x32 ks 3 z                           0.363
  convmid_fwd_train_x32 ks 3 sum z | sum z^2             0.123
  convmid_fwd_train ks 7 z                               0.295
  convmid_fwd_train ks 7 sum z | sum z^2                 0.0827
  convmid_fwd_train_x32 ks 7 z                           0.268
  convmid_fwd_train_x32 ks 7 sum z | sum z^2             0.102
  convmid_fwd_train ks 15 z                              0.197
  convmid_fwd_train ks 15 sum z | sum z^2                0.106
  convmid_fwd_train_x32 ks 15 z                          0.168
  convmid_fwd_train_x32 ks 15 sum z | sum z^2            0.106
  convmid_fwd_train ks 31 z                              0.106
  convmid_fwd_train ks 31 sum z | sum z^2                0.0883
  convmid_fwd_train_x32 ks 31 z                          0.107
  convmid_fwd_train_x32 ks 31 sum z | sum z^2            0.0866
  bn_swish_fwd C 256 / 512: outputs != RNE(float64 value) 0 of 36 096 / 72 192 (cap 0.5 %), none beyond one bf16 step
  bn_swish_fwd_x32 C 256 / 512                           0.353 / 0.378
  bn_finalize on convmid_fwd_train's partials 3 x 47 / 64 x 255 (compensated sums, double finalize)   0.437 / 0.294 of the tightened bound
  bn_swish_bwd (dn, dsum, d_gamma, d_beta, two-launch dz, _x32 dz; one-hot dsum exact), rows 1 / 7 / 1030:
    C 256 / 512 / 768 / 1024, 4-channel kernel           0.342 0.264 0.353 / 0.368 0.309 0.34 / 0.348 0.331 0.373 / 0.343 0.307 0.369
    C 256, scalar kernel                                 0.342 0.264 0.353
  convmid_bwd routing one-hots (_x32; strip edge 15 | 16, across utterances)                            exact
  convmid_bwd ks 3 / 7 / 15 / 31: dy bf16 (share != RNE / 0.5 %)   0.0158 / 0.0306 / 0.0521 / 0.0316   d_dw_w, d_dw_b 0.0482 / 0.0679 / 0.0642 / 0.149
  convmid_bwd_x32 ks 3 / 7 / 15 / 31: dy                           0.291 / 0.235 / 0.193 / 0.146       d_dw_w, d_dw_b 0.0474 / 0.0757 / 0.0705 / 0.154
  convmid_bwd per_block = 2 (B 700, T 33)                0.00501
  convmid_bwd_bn (fused) ks 15 T 47 / ks 3 T 17 / ks 31 T 5: dy   0.0277 / 0 / 0
  dense_join_splitk K = 1024                             exact
  dense_lnbwd(nxt=) g, dgamma, dbeta                     0.062    (dy_next exact)
  ffn_train_bwd g, dgamma, dbeta                         0.0718   (du from the gk tape and dy_next exact)
  conv1_dw with CMVN (exact without): staged C 256 / staged C 512, 468 positions / unstaged idim 2000 / scalar C 260
                                                         0.00305 / 0.00311 / 0.00185 / 0.00328
  adam n 1 / 4 / 1 048 580 / 4 194 308 (p, m, v; the mirror exact)   0 / 0.576 / 0.998 / 0.997
  sigmoid_fast(+40) = 1.0 (1 - it = 0): the bf16 mode's routing cases are bit-exact as well
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_kernel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

F32_SENTINEL = 0x7FC0BEEF
BF16_SENTINEL = 0xABCD - 0x10000


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from mindaudio_amd import _lib

    return _lib.load()


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(t):
    return t.contiguous().cuda() if t is not None else None


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


class Guard:
    """A (rows, cols) window with row stride ld inside a sentinel-filled device buffer: `top` rows above, `bottom` below, ld - cols
    guard columns behind every row.  ld % 8 == 0 keeps every row 16-byte aligned."""

    def __init__(self, rows, cols, dtype, ld=None, top=2, bottom=3, fill=None):
        self.rows, self.cols, self.top = rows, cols, top
        self.ld = ld if ld is not None else (cols + 7) // 8 * 8 + 8
        self.buf = torch.empty(top + rows + bottom, self.ld, dtype=dtype, device="cuda")
        self.sentinel = {4: F32_SENTINEL, 2: BF16_SENTINEL, 1: 0x5A}[self.buf.element_size()]
        bits(self.buf).fill_(self.sentinel)
        self.view = self.buf[top:top + rows, :cols]
        if fill is not None:
            self.view.copy_(fill.view(rows, cols))
        self.before = bits(self.buf).clone()

    def flat(self):
        assert self.rows == 1
        return self.view[0]

    def intact(self, owned=True):
        """Guards untouched; owned: every element of the window was written (no sentinel left).  -> None or a message."""
        now = bits(self.buf)
        changed = now != self.before
        changed[self.top:self.top + self.rows, :self.cols] = False
        if bool(changed.any()):
            r, c = [int(v) for v in changed.nonzero()[0]]
            return "guard overwritten at buffer row %d (window row %d of %d), column %d of %d (window %d)" % (
                r, r - self.top, self.rows, c, self.ld, self.cols)
        if owned:
            left = bits(self.view) == self.sentinel
            if bool(left.any()):
                return "%d owned elements not written, first at %s" % (int(left.sum()), tuple(int(v) for v in left.nonzero()[0]))
        return None

    def untouched(self):
        return bool((bits(self.buf) == self.before).all())


def vec(n, dtype, fill=None):
    return Guard(1, n, dtype, fill=fill)


def report(name, worst, pos):
    print("%-58s worst error / bound %.3g" % (name, worst))
    assert worst <= 1 and not pos, (name, worst, pos)


# ---- dropout sites -----------------------------------------------------------------------------------------------------------------
P_SS = [(p, ss) for p in T.DROP_PS + (T.P_TINY,) for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]


@pytest.mark.parametrize("bwd", (False, True))
@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("act", (T.ACT_SWISH, T.ACT_RELU))
def test_act_dropout_sites(L, act, x32, bwd):
    n = 1001 if x32 else 5 * 264
    dt = torch.float32 if x32 else torch.bfloat16
    worst = 0.0
    for p, (seed, salt) in P_SS:
        c = T.act_dropout_case(n, act, p, seed, salt, x32, bwd)
        u, dh, out = dev(c["u"].to(dt)), dev(c["dh"].to(dt)), vec(n, dt)
        fwd, bk = (L.ma_act_dropout_fwd_x32, L.ma_act_dropout_bwd_x32) if x32 else (L.ma_act_dropout_fwd_bf16, L.ma_act_dropout_bwd_bf16)
        if bwd:
            rc = bk(P(u), P(dh), P(out.flat()), n, act, p, seed, salt, st())
        else:
            rc = fwd(P(u), P(out.flat()), n, act, p, seed, salt, st())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() is None, (rc, out.intact())
        w, pos = T.check_drop_site(out.flat(), c)
        assert w <= 1 and not pos, (p, seed, salt, w, pos)
        worst = max(worst, w)
        if p in T.DROP_PS:  # the mask is not trivially all-kept: the restated fraction is what the device dropped
            assert 0 < int((out.flat() == 0).sum()) < n
    report("act_dropout %s %s %s" % ("swish" if act == T.ACT_SWISH else "relu", "x32" if x32 else "bf16", "bwd" if bwd else "fwd"), worst, [])


@pytest.mark.parametrize("y_bf16", (False, True))
@pytest.mark.parametrize("cols", (256, 264))
def test_dropout_add_sites(L, cols, y_bf16):
    rows = 5
    for i, (p, (seed, salt)) in enumerate(P_SS):
        with_x = i != 1  # x = None once
        c = T.dropout_add_case(rows, cols, y_bf16, with_x, p, seed, salt)
        y = dev(c["y"])
        out = Guard(rows, cols, torch.float32, ld=cols + 8)
        xin = Guard(rows, cols, torch.float32, ld=cols + 8, fill=c["x"]) if with_x else None
        rc = L.ma_dropout_add_f32(P(out.view), out.ld, P(xin.view) if with_x else None, xin.ld if with_x else 0, P(y), y.stride(0),
                                  1 if y_bf16 else 0, rows, cols, c["alpha"], p, seed, salt, st())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() is None and (xin is None or xin.untouched()), (rc, out.intact())
        w, pos = T.check_exact(out.view.cpu(), c)
        assert w == 0, (p, seed, salt, with_x, pos)
        if with_x:  # the in-place form (out = x) gives the same bits
            rc = L.ma_dropout_add_f32(P(xin.view), xin.ld, P(xin.view), xin.ld, P(y), y.stride(0), 1 if y_bf16 else 0, rows, cols,
                                      c["alpha"], p, seed, salt, st())
            torch.cuda.synchronize()
            assert rc == 0 and xin.intact() is None and T.check_exact(xin.view.cpu(), c)[0] == 0


@pytest.mark.parametrize("x32", (False, True))
def test_dropout_bwd_sites(L, x32):
    rows = 5
    dt = torch.float32 if x32 else torch.bfloat16
    for i, (p, (seed, salt)) in enumerate(P_SS):
        cols = (256, 264)[i % 2]
        c = T.dropout_bwd_case(rows, cols, x32, p, seed, salt)
        g = Guard(rows, cols, torch.float32, ld=cols + 8, fill=c["g"])
        dy = Guard(rows, cols, dt, ld=cols + 8)
        fn = L.ma_dropout_bwd_x32 if x32 else L.ma_dropout_bwd_bf16
        rs = dev(c["row_scale"])
        rc = fn(P(g.view), g.ld, P(dy.view), dy.ld, rows, cols, c["alpha"], P(rs), p, seed, salt, st())
        torch.cuda.synchronize()
        assert rc == 0 and dy.intact() is None and g.untouched(), (rc, dy.intact())
        w, pos = T.check_drop_site(dy.view, c)
        assert w <= 1 and not pos, (p, seed, salt, pos)


# ---- dropout sites in the GEMM epilogues -------------------------------------------------------------------------------------------
def pack(L, w, kind):
    """The batched packer on one (n, k) bf16 weight: kind 0 = the K = 256 layout, 1 = the rows layout."""
    from mindaudio_amd import _lib

    n, k = w.shape
    pieces = int(L.ma_pack_item_pieces(kind, n, k))
    assert pieces > 0
    out = torch.empty(pieces * 16, dtype=torch.uint8, device="cuda")
    items = (_lib.PackItem * 1)(_lib.PackItem(w.data_ptr(), out.data_ptr(), w.stride(0), n, k, kind, 0))
    d_items = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).cuda()
    d_map = torch.zeros((pieces + 255) // 256, dtype=torch.int32, device="cuda")
    assert L.ma_pack_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), d_map.numel(), st()) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("bwd", (False, True))
@pytest.mark.parametrize("act", (T.ACT_SWISH, T.ACT_RELU))
def test_dense_act_drop_sites(L, act, bwd):
    """dense_act_drop / dense_act_drop_bwd (ma_gemm_k256_train_bf16 modes 1 / 2), m = 70, n = 512: element index mc * N + n."""
    from mindaudio_amd.train import kernels as K

    m, n = T.GEMM_M, T.GEMM_N
    worst = 0.0
    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        c = T.dense_act_case(act, bwd, p, seed, salt)
        a, pk = dev(c["a"]), pack(L, dev(c["w"]), 0)
        out, u = Guard(m, n, torch.bfloat16, ld=n + 8), Guard(m, n, torch.bfloat16, ld=n + 8, fill=c["u"] if bwd else None)
        if bwd:
            e = K._train_epi(2, aux=u.view, p=p, seed=seed, salt=salt)
            dst = out
        else:
            bias = dev(c["bias"])
            e = K._train_epi(1, bias=bias, out2=out.view, p=p, seed=seed, salt=salt)
            dst = u
        e.act = 2 if act == T.ACT_RELU else 0
        rc = L.ma_gemm_k256_train_bf16(P(a), a.stride(0), P(pk), P(dst.view), dst.ld, m, n, ctypes.byref(e), st())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() is None and (u.untouched() if bwd else u.intact() is None), (rc, out.intact(), u.intact())
        if not bwd:
            assert torch.equal(bits(u.view.cpu()), bits(c["u"]))  # the pre-activation: an exact integer
        w, pos = T.check_drop_site(out.view, c)
        assert w <= 1 and not pos, (p, seed, salt, w, pos)
        worst = max(worst, w)
    report("dense_act_drop%s %s" % ("_bwd" if bwd else "", "swish" if act == T.ACT_SWISH else "relu"), worst, [])


@pytest.mark.parametrize("k", (256, 512))
def test_dense_join_sites(L, k):
    """dense_join through ma_gemm_k256_train_bf16 (k = 256) and ma_gemm_rows_train_bf16 (k = 512), m = 70: index mc * 256 + n."""
    from mindaudio_amd.train import kernels as K

    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        c = T.dense_join_case(k, p, seed, salt)
        a, pk = dev(c["a"]), pack(L, dev(c["w"]), 0 if k == 256 else 1)
        bias, res, rs = dev(c["bias"]), dev(c["residual"]), dev(c["row_scale"])
        m = c["m"]
        out = Guard(m, 256, torch.float32, ld=264)
        e = K._train_epi(3, bias=bias, residual=res, row_scale=rs, alpha=c["alpha"], p=p, seed=seed, salt=salt)
        if k == 256:
            rc = L.ma_gemm_k256_train_bf16(P(a), a.stride(0), P(pk), P(out.view), out.ld, m, 256, ctypes.byref(e), st())
        else:
            rc = L.ma_gemm_rows_train_bf16(P(a), a.stride(0), m, k, P(pk), P(out.view), out.ld, ctypes.byref(e), st())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() is None, (rc, out.intact())
        w, pos = T.check_exact(out.view.cpu(), c)
        assert w == 0, (k, p, seed, salt, pos)
        assert torch.equal(res.cpu(), c["residual"])


def test_ffn_train_sites(L):
    """Both dropout sites of ma_ffn_train_bf16 (hidden: mc * hidden + n, join: mc * 256 + n) and the gk tape, m = 70, hidden = 256."""
    from mindaudio_amd import ops
    from mindaudio_amd.train import kernels as K

    worst = 0.0
    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        sh, sj = salt, (salt + 1) & 0xFFFFFFFF
        c = T.ffn_train_case(p, p, seed, sh, sj)
        a, w1, w2 = dev(c["a"]), dev(c["w1"]), dev(c["w2"])
        pk = ops.ffn_pack_weights(w1, w2)
        b1, b2, res = dev(c["b1"]), dev(c["b2"]), dev(c["residual"])
        m, hid = c["m"], c["hidden"]
        outs = []
        for tape_derivative in (0, 1):
            u, h = Guard(m, hid, torch.bfloat16, ld=hid + 8), Guard(m, hid, torch.bfloat16, ld=hid + 8)
            xo = Guard(m, 256, torch.float32, ld=264)
            e = K._train_epi(3, bias=b2, residual=res, alpha=c["alpha"], p=p, seed=seed, salt=sj)
            rc = L.ma_ffn_train_bf16(P(a), a.stride(0), m, hid, P(pk), P(b1), P(u.view), P(h.view), u.ld, tape_derivative, p, seed, sh,
                                     P(xo.view), xo.ld, ctypes.byref(e), st())
            torch.cuda.synchronize()
            assert rc == 0, rc
            for gd in (u, h, xo):
                assert gd.intact() is None, gd.intact()
            outs.append((u.view.cpu(), h.view.cpu(), xo.view.cpu()))
        (u, h, xo), (gk, h2, xo2) = outs
        assert torch.equal(bits(u), bits(c["u"])) and torch.equal(bits(h), bits(h2)) and torch.equal(bits(xo), bits(xo2))
        for name, got in (("h", h), ("gk", gk)):
            w, pos = T.check_drop_site(got, c[name])
            assert w <= 1 and not pos, (name, p, seed, salt, w, pos)
            worst = max(worst, w)
        w, pos = T.check_exact(xo, T.ffn_join_want(c, h))
        assert w == 0, ("join", p, seed, salt, pos)
    report("ffn_train hidden site h, gk tape (join site exact)", worst, [])


def test_dense_join_splitk_site(L):
    """ma_gemm_bf16_splitk_join_f32, m = 70, K = 1024: the join's dropout at index mc * 256 + n, exact on integer operands."""
    from mindaudio_amd.train import kernels as K

    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        c = T.dense_join_case(T.SPLITK_K, p, seed, salt, with_rs=False)
        m, k = c["m"], T.SPLITK_K
        a, w, bias, res = dev(c["a"]), dev(c["w"]), dev(c["bias"]), dev(c["residual"])
        out = Guard(m, 256, torch.float32, ld=264)
        nbytes = int(L.ma_gemm_splitk_workspace_bytes(m, 256, k))
        ws = vec(nbytes // 4, torch.float32)  # exactly the bytes the launcher asks for
        e = K._train_epi(3, bias=bias, residual=res, alpha=c["alpha"], p=p, seed=seed, salt=salt)
        rc = L.ma_gemm_bf16_splitk_join_f32(P(a), a.stride(0), P(w), w.stride(0), P(out.view), out.ld, m, 256, k, ctypes.byref(e),
                                            P(ws.flat()), nbytes, st())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() is None and ws.intact(owned=False) is None, (rc, out.intact(), ws.intact(owned=False))
        w_, pos = T.check_exact(out.view.cpu(), c)
        assert w_ == 0, (p, seed, salt, pos)


def _epi5(x, gamma, parts, dyn=None, nxt=None, row_scale=None):
    """ma_train_epilogue_t of mode 5 (the LayerNorm backward in a product's epilogue)."""
    from mindaudio_amd import _lib

    e = _lib.TrainEpilogue()
    e.mode = 5
    e.residual, e.ldr = x.data_ptr(), x.stride(0)
    e.ln_gamma1, e.ln_eps, e.ln_mid = gamma.data_ptr(), T.EPS_LN, parts.data_ptr()
    e.row_scale = row_scale.data_ptr() if row_scale is not None else None
    if nxt is not None:
        alpha, p, seed, salt, rs2 = nxt
        e.ln_out, e.ld_ln, e.ln_out_bf16 = dyn.data_ptr(), dyn.stride(0), 1
        e.alpha, e.p, e.seed, e.salt = alpha, p, seed, salt
        e.ln_row_scale = rs2.data_ptr() if rs2 is not None else None
    return e


def test_dense_lnbwd_site(L):
    """dense_lnbwd(nxt=): ma_gemm_rows_train_bf16 mode 5, m = 70, K = 512: g, the partial (dgamma | dbeta) vectors, and dy_next equal
    to the restated mask at index mc * 256 + n on the g rows the launch stored."""
    c = T.dense_lnbwd_case()
    m, k = c["m"], c["k"]
    a, pk = dev(c["a"]), pack(L, dev(c["w"]), 1)
    gamma, rs = dev(c["gamma"]), dev(c["row_scale"])
    rs2 = torch.tensor([1.0, 0.0, 0.5])[torch.randint(0, 3, (m,), generator=torch.Generator().manual_seed(5))]
    rs2d = dev(rs2)
    nparts = int(L.ma_gemm_rows_train_parts(m))
    worst = 0.0
    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        x = Guard(m, 256, torch.float32, ld=260, fill=c["x"])
        g = Guard(m, 256, torch.float32, ld=260, fill=c["g0"])
        dyn = Guard(m, 256, torch.bfloat16, ld=264)
        parts = Guard(nparts, 512, torch.float32, ld=512, top=1, bottom=1)
        e = _epi5(x.view, gamma, parts.view, dyn.view, (0.5, p, seed, salt, rs2d), rs)
        rc = L.ma_gemm_rows_train_bf16(P(a), a.stride(0), m, k, P(pk), P(g.view), g.ld, ctypes.byref(e), st())
        torch.cuda.synchronize()
        assert rc == 0 and x.untouched(), rc
        for gd in (g, dyn, parts):
            assert gd.intact() is None, gd.intact()
        tot = parts.view.double().sum(0).cpu()
        w, pos = T.check_ln_bwd((g.view.cpu(), tot[:256], tot[256:]), c)
        assert w <= 1 and not pos, (p, w, pos)
        worst = max(worst, w)
        w, pos = T.check_drop_site(dyn.view, T.dy_next_case(g.view.cpu(), 0.5, rs2, p, seed, salt))
        assert w <= 1 and not pos, ("dy_next", p, seed, salt, pos)
    report("dense_lnbwd(nxt=) g, dgamma, dbeta (dy_next exact)", worst, [])


def test_ffn_train_bwd_reads_the_tape(L):
    """The consumer of the gk tape: ma_ffn_train_bf16 (tape_derivative) writes gk, ma_ffn_train_bwd_bf16 reads it.  du must be
    bf16(bf16(dy W2) gk) of the tape bit for bit (so a consumer that regenerated or indexed the mask differently cannot pass), g and the
    partial vectors the LayerNorm backward of bf16(du W1), dy_next the restated mask on the stored g."""
    from mindaudio_amd import ops
    from mindaudio_amd.train import kernels as K

    bc = T.ffn_bwd_case()
    m, hid = bc["m"], bc["hidden"]
    dy = dev(bc["dy"])
    pkt = ops.ffn_pack_weights(dev(bc["w2t"]), dev(bc["w1t"]))
    gamma = dev(bc["gamma"])
    nparts = int(L.ma_ffn_train_parts(m))
    worst = 0.0
    for p, (seed, salt) in [(q, ss) for q in T.DROP_PS for ss in T.SEED_SALTS] + [(0.0, T.SEED_SALTS[0])]:
        sh, sj = salt, (salt + 1) & 0xFFFFFFFF
        fc = T.ffn_train_case(p, p, seed, sh, sj)
        a, b1, b2, res = dev(fc["a"]), dev(fc["b1"]), dev(fc["b2"]), dev(fc["residual"])
        pk = ops.ffn_pack_weights(dev(fc["w1"]), dev(fc["w2"]))
        gk, h = Guard(m, hid, torch.bfloat16, ld=hid + 8), Guard(m, hid, torch.bfloat16, ld=hid + 8)
        xo = Guard(m, 256, torch.float32, ld=264)
        e = K._train_epi(3, bias=b2, residual=res, alpha=fc["alpha"], p=p, seed=seed, salt=sj)
        rc = L.ma_ffn_train_bf16(P(a), a.stride(0), m, hid, P(pk), P(b1), P(gk.view), P(h.view), gk.ld, 1, p, seed, sh, P(xo.view), xo.ld,
                                 ctypes.byref(e), st())
        torch.cuda.synchronize()
        assert rc == 0 and gk.intact() is None, (rc, gk.intact())
        w, pos = T.check_drop_site(gk.view, fc["gk"])
        assert w <= 1 and not pos, ("gk", p, seed, salt, pos)
        tape = gk.view.cpu()
        gk.before = bits(gk.buf).clone()
        du_want, ln = T.ffn_bwd_want(bc, tape)
        du = Guard(m, hid, torch.bfloat16, ld=hid + 8)
        x = Guard(m, 256, torch.float32, ld=260, fill=bc["x"])
        g = Guard(m, 256, torch.float32, ld=260, fill=bc["g0"])
        dyn = Guard(m, 256, torch.bfloat16, ld=264)
        parts = Guard(nparts, 512, torch.float32, ld=512, top=1, bottom=1)
        e5 = _epi5(x.view, gamma, parts.view, dyn.view, (0.5, p, seed, sj, None))
        rc = L.ma_ffn_train_bwd_bf16(P(dy), dy.stride(0), m, hid, P(pkt), P(gk.view), P(du.view), du.ld, P(g.view), g.ld,
                                     ctypes.byref(e5), None, st())
        torch.cuda.synchronize()
        assert rc == 0 and gk.untouched() and x.untouched(), rc
        for gd in (du, g, dyn, parts):
            assert gd.intact() is None, gd.intact()
        w, pos = T.check_exact(du.view.cpu(), {"want": du_want})
        assert w == 0, ("du", p, seed, salt, pos)
        tot = parts.view.double().sum(0).cpu()
        w, pos = T.check_ln_bwd((g.view.cpu(), tot[:256], tot[256:]), ln)
        assert w <= 1 and not pos, (p, w, pos)
        worst = max(worst, w)
        w, pos = T.check_drop_site(dyn.view, T.dy_next_case(g.view.cpu(), 0.5, None, p, seed, sj))
        assert w <= 1 and not pos, ("dy_next", p, seed, salt, pos)
    report("ffn_train_bwd g, dgamma, dbeta (du from the tape and dy_next exact)", worst, [])


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------
def run_ln_bwd(L, c, partials=False, nxt=None):
    """-> (g, dgamma, dbeta[, dy_next]) as the launch left them, after the guard checks."""
    rows, D = c["rows"], c["D"]
    ld = D + 4
    x = Guard(rows, D, torch.float32, ld=ld, fill=c["x"])
    g = Guard(rows, D, torch.float32, ld=ld, fill=c["g0"])
    dy = g.view if c["inplace"] else dev(c["dy"].bfloat16() if c["dy_bf16"] else c["dy"])
    dg, db = vec(D, torch.float32, fill=c["dg0"]), vec(D, torch.float32, fill=c["db0"])
    parts = int(L.ma_layernorm_bwd_parts(rows))
    assert parts == min((rows + 3) // 4, T.LN_BLOCKS)
    ws = Guard(parts, 2 * D, torch.float32, ld=2 * D, top=1, bottom=1)  # exactly the bytes the launcher asks for
    gamma, rs = dev(c["gamma"]), dev(c["row_scale"])  # (named: a temporary's memory is handed to the next allocation)
    args = [P(x.view), ld, rows, D, P(gamma), T.EPS_LN, P(rs), P(dy), dy.stride(0), 1 if c["dy_bf16"] else 0,
            P(g.view), ld, 1 if c["accumulate"] else 0, None if partials else P(dg.flat()), None if partials else P(db.flat()), P(ws.view),
            parts * 2 * D * 4]
    if nxt is None:
        rc = L.ma_layernorm_bwd_f32(*args, st())
    else:
        alpha, p, seed, salt, rs2 = nxt
        dyn = Guard(rows, 256, torch.bfloat16, ld=264)
        rs2 = dev(rs2)
        rc = L.ma_layernorm_bwd_next_f32(*args, P(dyn.view), dyn.ld, alpha, P(rs2), p, seed, salt, st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert g.intact() is None and x.untouched() and ws.intact() is None, (g.intact(), ws.intact())
    if partials:
        assert dg.untouched() and db.untouched()
        tot = ws.view.double().sum(0).cpu()
        out = (g.view.cpu(), tot[:D], tot[D:])
    else:
        assert dg.intact() is None and db.intact() is None
        out = (g.view.cpu(), dg.flat().cpu(), db.flat().cpu())
    if nxt is not None:
        assert dyn.intact() is None, dyn.intact()
        out += (dyn.view.cpu(),)
    return out


LN_GRID = [(rows, D, dy_bf16, acc) for rows in T.LN_ROWS for D in T.LN_WIDTHS for dy_bf16 in (False, True) for acc in (False, True)
           if rows != 4099 or (dy_bf16, acc) in ((False, True), (True, False))]


@pytest.mark.parametrize("rows,D,dy_bf16,acc", LN_GRID)
def test_layernorm_bwd(L, rows, D, dy_bf16, acc):
    c = T.ln_bwd_case(rows, D, dy_bf16, acc)
    report("layernorm_bwd rows %d D %d %s %s" % (rows, D, "bf16" if dy_bf16 else "f32", "acc" if acc else "store"),
           *T.check_ln_bwd(run_ln_bwd(L, c), c))
    cp = dict(c, partials=True)
    report("layernorm_bwd partials= rows %d D %d" % (rows, D), *T.check_ln_bwd(run_ln_bwd(L, cp, partials=True), cp))


@pytest.mark.parametrize("D", T.LN_WIDTHS)
def test_layernorm_bwd_inplace_and_onehot(L, D):
    c = T.ln_bwd_case(5, D, False, False, inplace=True)
    report("layernorm_bwd in place D %d" % D, *T.check_ln_bwd(run_ln_bwd(L, c), c))
    for r in (0, 4098, 4097):  # the first row, the last row, a row of the wrapped round
        c = T.ln_bwd_case(4099, D, True, True, onehot=r)
        report("layernorm_bwd one-hot row %d D %d" % (r, D), *T.check_ln_bwd(run_ln_bwd(L, c), c))


@pytest.mark.parametrize("rows", (5, 4099))
def test_layernorm_bwd_next_site(L, rows):
    c = T.ln_bwd_case(rows, 256, True, True)
    rs2 = torch.tensor([1.0, 0.0, 0.5])[torch.randint(0, 3, (rows,), generator=torch.Generator().manual_seed(rows))]
    rs2[0], rs2[1] = 1.0, 0.0
    worst = 0.0
    for i, (p, (seed, salt)) in enumerate(P_SS):
        partials = i % 2 == 1
        cc = dict(c, partials=partials)
        g, dg, db, dyn = run_ln_bwd(L, cc, partials=partials, nxt=(0.5, p, seed, salt, rs2 if i != 2 else None))
        w, pos = T.check_ln_bwd((g, dg, db), cc)
        assert w <= 1 and not pos, (p, w, pos)
        worst = max(worst, w)
        site = T.dy_next_case(g, 0.5, rs2 if i != 2 else None, p, seed, salt)
        w, pos = T.check_drop_site(dyn, site)
        assert w <= 1 and not pos, ("dy_next", p, seed, salt, pos)
    report("layernorm_bwd_next rows %d (g, dgamma, dbeta; dy_next exact)" % rows, worst, [])


# ---- BatchNorm finalize ------------------------------------------------------------------------------------------------------------
def run_bn_finalize(L, c):
    C = c["C"]
    sums = Guard(c["nparts"], 2 * C, torch.float32, ld=2 * C, top=1, bottom=1, fill=c["sums"])
    stats = vec(2 * C, torch.float32)
    rm, rv = vec(C, torch.float32, fill=c["run_mean"]), vec(C, torch.float32, fill=c["run_var"])
    rc = L.ma_bn_finalize_f32(P(sums.view), c["nparts"], C, c["count"], T.BN_EPS, T.BN_MOMENTUM, P(rm.flat()), P(rv.flat()), P(stats.flat()),
                              st())
    torch.cuda.synchronize()
    assert rc == 0 and sums.untouched()
    for gd in (stats, rm, rv):
        assert gd.intact() is None, gd.intact()
    return stats.flat().cpu(), rm.flat().cpu(), rv.flat().cpu()


@pytest.mark.parametrize("C", T.BN_CS)
def test_bn_finalize(L, C):
    worst = 0.0
    for nparts in T.BN_NPARTS:
        c = T.bn_finalize_case(nparts, C)
        w, pos = T.check_bn_finalize(run_bn_finalize(L, c), c)
        assert w <= 1 and not pos, (nparts, w, pos)
        worst = max(worst, w)
    c = T.bn_finalize_case(1, C, count=1)
    w, pos = T.check_bn_finalize(run_bn_finalize(L, c), c)
    report("bn_finalize C %d (nparts %s, count = 1)" % (C, "/".join(str(n) for n in T.BN_NPARTS)), max(worst, w), pos)


# ---- training conv module, forward -------------------------------------------------------------------------------------------------
def run_convmid_fwd(L, c, x32):
    """-> (z (B T, C), partial vectors (nparts, 2 C)) of ma_convmid_fwd_train / _x32 with ldy = 2 C + 8, after the guard checks."""
    B, Tn, C, ks = c["B"], c["T"], c["C"], c["ks"]
    y = Guard(B * Tn, 2 * C, torch.float32 if x32 else torch.bfloat16, ld=2 * C + 8, fill=c["y"])
    w, bias = dev(c["w"]), dev(c["bias"])
    nparts = int(L.ma_convmid_fwd_train_parts(B, Tn, C))
    assert nparts == B * ((Tn + 31) // 32)
    z = Guard(B * Tn, C, torch.float32, ld=C)
    sums = Guard(nparts, 2 * C, torch.float32, ld=2 * C, top=1, bottom=1)
    fn = L.ma_convmid_fwd_train_x32 if x32 else L.ma_convmid_fwd_train
    rc = fn(P(y.view), y.ld, B, Tn, C, P(w), ks, P(bias), P(z.view), P(sums.view), st())
    torch.cuda.synchronize()
    assert rc == 0 and y.untouched() and z.intact() is None and sums.intact() is None, (rc, z.intact(), sums.intact())
    return z.view.cpu(), sums.view.cpu()


def test_fast_sigmoid_at_40(L):
    """What the bf16 mode's sigmoid_fast returns at +40, read through the forward kernel: a = 1, centre tap 1, bias 0 -> z = sigmoid."""
    C = 256
    y = torch.zeros(1, 2 * C)
    y[0, :C], y[0, C:] = 1.0, 40.0
    w = torch.zeros(C, 3)
    w[:, 1] = 1.0
    z, _ = run_convmid_fwd(L, {"y": y.bfloat16(), "B": 1, "T": 1, "C": C, "ks": 3, "w": w, "bias": torch.zeros(C)}, False)
    print("sigmoid_fast(+40) = %r (1 - it = %.3g)" % (float(z[0, 0]), 1.0 - float(z[0, 0].double())))
    assert float(z.min()) == float(z.max()) and abs(1.0 - float(z[0, 0])) <= 2 * T.U


@pytest.mark.parametrize("C", T.CONV_CS)
@pytest.mark.parametrize("ks", T.CONV_KS)
def test_convmid_fwd_routing(L, ks, C):
    for Tn in T.CONV_TS:
        for x32 in (True, False):
            c = T.conv_route_case(ks, Tn, C, x32)
            z, _ = run_convmid_fwd(L, c, x32)
            w, pos = T.check_exact(z, c)
            if w and not x32:  # only if the fast sigmoid is not exactly 1 at +40 (test_fast_sigmoid_at_40 prints it): 2 u |z|
                w, pos = T.check_bound(z, {"want": c["want"].double(), "bound": 2 * T.U * c["want"].double().abs()})
            assert w <= 1 and not pos, (ks, Tn, C, x32, pos)
            mid = z.view(3, Tn, C)[1]
            assert torch.equal(mid, c["bias"].expand(Tn, C))  # the all-zero middle utterance: the bias exactly


@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("ks", T.CONV_KS)
def test_convmid_fwd_random(L, ks, x32):
    worst_z = worst_s = 0.0
    for Tn in T.CONV_TS:
        for C in T.CONV_CS:
            c = T.conv_random_case(ks, Tn, C, x32)
            want, bound = T.conv_z_bound(c)
            z, sums = run_convmid_fwd(L, c, x32)
            w, pos = T.check_bound(z, {"want": want, "bound": bound})
            assert w <= 1 and not pos, ("z", ks, Tn, C, w, pos)
            w2, pos = T.check_bound(sums.double().sum(0), T.conv_sums_bound(z, c["B"], Tn, C))
            assert w2 <= 1 and not pos, ("sums", ks, Tn, C, w2, pos)
            worst_z, worst_s = max(worst_z, w), max(worst_s, w2)
    report("convmid_fwd_train%s ks %d z" % ("_x32" if x32 else "", ks), worst_z, [])
    report("convmid_fwd_train%s ks %d sum z | sum z^2" % ("_x32" if x32 else "", ks), worst_s, [])


@pytest.mark.parametrize("B,Tn", ((3, 47), (64, 255)))
def test_bn_one_pass_variance(L, B, Tn):
    """var = E[z^2] - mean^2 with |mean| / sigma in {0, 4, 32} (through the depthwise bias): stats against the float64 statistics of the z
    the launch stored, per channel, within the bound derived from the kernels' arithmetic (compensated float32 sums in the forward
    workgroup, double in the finalize), which stays below 2^-9 relative in rstd at every ratio.  Measured relative error of rstd on an
    MI355X / the derived bound:
        3 x 47     ratio 0: 1.0e-7 / 6.9e-7    4: 4.5e-7 / 4.0e-6    32: 4.1e-5 / 2.2e-4
        64 x 255   ratio 0: 1.0e-7 / 6.9e-7   4: 1.1e-7 / 4.0e-6   32: 3.5e-6 / 2.2e-4
    (with float32 chains and a float32 subtraction: 2.7e-4 measured, 7.8e-3 = 2^-7 derived at ratio 32 over 16 320 frames)."""
    C = 256
    ratio = torch.tensor([0.0, 4.0, 32.0])[torch.arange(C) % 3]
    c = T.conv_random_case(15, Tn, C, False, B=B, bias_ratio=ratio)
    z, sums = run_convmid_fwd(L, c, False)
    oc = T.bn_onepass_case(sums, z, B * Tn, C)
    got = run_bn_finalize(L, dict(oc, sums=sums))
    want, bound = oc["stats"]["want"][C:], oc["stats"]["bound"][C:]
    rel = ((got[0][C:].double() - want) / want).abs()
    zd = z.double()
    real = (zd.mean(0) / zd.std(0, unbiased=False)).abs()
    for k, r in enumerate((0, 4, 32)):
        print("one-pass variance %d x %d |mean|/sigma %2d (realised %.1f .. %.1f): rstd relative error %.3g, derived bound %.3g" % (
            B, Tn, r, float(real[k::3].min()), float(real[k::3].max()), float(rel[k::3].max()), float((bound / want)[k::3].max())))
    assert float((bound / want).max()) < 2.0 ** -9
    report("bn_finalize on convmid_fwd_train's partials %d x %d" % (B, Tn), *T.check_bn_finalize(got, oc))


@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("C", T.CONV_CS)
def test_bn_swish_fwd_out(L, C, x32):
    """out = swish(gamma (z - mean) rstd + beta): bf16 within one bf16 step of the float64 value and at most 0.5 % of the elements
    different from its round-to-nearest-even; _x32 within the float32 bound.  rows = 141 = 3 x 47."""
    c = T.bn_swish_fwd_case(141, C, x32)
    z, stats, gamma, beta = dev(c["z"]), dev(c["stats"]), dev(c["gamma"]), dev(c["beta"])
    out = Guard(141, C, torch.float32 if x32 else torch.bfloat16, ld=C)
    fn = L.ma_bn_swish_fwd_x32 if x32 else L.ma_bn_swish_fwd_bf16
    rc = fn(P(z), P(stats), P(gamma), P(beta), P(out.view), 141, C, st())
    torch.cuda.synchronize()
    assert rc == 0 and out.intact() is None, (rc, out.intact())
    report("bn_swish_fwd%s C %d%s" % ("_x32" if x32 else "", C, "" if x32 else " (share of outputs != RNE(float64) / 0.5 %)"),
           *T.check_bn_swish_out(out.view, c))


# ---- training conv module, backward ------------------------------------------------------------------------------------------------
def run_bn_swish_bwd(L, c, stage1_only=False, scalar=False):
    """ma_bn_swish_bwd_f32 / _x32 (two launches: dz) or ma_bn_swish_bwd_stage1_f32 (dn) -> (dn or dz, dsum, d_gamma, d_beta, dg0, db0).
    scalar: dz starts one float behind a 16-byte boundary, which selects the kernel that issues scalar accesses only."""
    rows, C, x32 = c["rows"], c["C"], c["x32"]
    dout = dev(c["dout"] if x32 else c["dout"].bfloat16())
    z, stats, gamma, beta = dev(c["z"]), dev(c["stats"]), dev(c["gamma"]), dev(c["beta"])
    off = 1 if scalar else 0
    dz = vec(rows * C + off, torch.float32)
    g = torch.Generator().manual_seed(C + rows)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dsum, dg, db = vec(2 * C, torch.float32), vec(C, torch.float32, fill=dg0), vec(C, torch.float32, fill=db0)
    ws = torch.empty(T.BN_BWD_BLOCKS * 2 * C, device="cuda")
    fn = L.ma_bn_swish_bwd_stage1_f32 if stage1_only else (L.ma_bn_swish_bwd_x32 if x32 else L.ma_bn_swish_bwd_f32)
    assert not (stage1_only and x32)
    rc = fn(P(dout), P(z), P(stats), P(gamma), P(beta), P(dz.flat()[off:]), rows, C, P(dsum.flat()), P(dg.flat()), P(db.flat()), P(ws),
            ws.numel() * 4, st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for gd in (dz, dsum, dg, db):
        assert gd.intact(owned=gd is not dz) is None, gd.intact()
    assert not bool((bits(dz.flat()[off:]) == F32_SENTINEL).any())
    assert off == 0 or int(bits(dz.flat())[0]) == F32_SENTINEL  # the float in front of the misaligned window
    return dz.flat()[off:].view(rows, C).cpu(), dsum.flat().cpu(), dg.flat().cpu(), db.flat().cpu(), dg0, db0


@pytest.mark.parametrize("rows", T.BN_BWD_ROWS)
@pytest.mark.parametrize("C,scalar", ((256, False), (512, False), (768, False), (1024, False), (256, True)))
def test_bn_swish_bwd(L, C, scalar, rows):
    c = T.bn_swish_bwd_case(rows, C)
    worst = 0.0
    dn, dsum, dg, db, dg0, db0 = run_bn_swish_bwd(L, c, stage1_only=True, scalar=scalar)
    for name, got, case in (("dn", dn, c["dn"]), ("dsum", dsum, c["dsum"]),
                            ("d_beta", db, {"want": db0.double() + c["dsum"]["want"][:C],
                                            "bound": c["dsum"]["bound"][:C] + 2 * T.U * (db0.double() + c["dsum"]["want"][:C]).abs()}),
                            ("d_gamma", dg, {"want": dg0.double() + c["dsum"]["want"][C:],
                                             "bound": c["dsum"]["bound"][C:] + 2 * T.U * (dg0.double() + c["dsum"]["want"][C:]).abs()})):
        w, pos = T.check_bound(got, case)
        assert w <= 1 and not pos, (name, w, pos)
        worst = max(worst, w)
    dz = run_bn_swish_bwd(L, c, scalar=scalar)[0]
    w, pos = T.check_bound(dz, c["dz"])
    assert w <= 1 and not pos, ("dz", w, pos)
    worst = max(worst, w)
    if not scalar:
        cx = T.bn_swish_bwd_case(rows, C, x32=True)
        w, pos = T.check_bound(run_bn_swish_bwd(L, cx)[0], cx["dz"])
        assert w <= 1 and not pos, ("dz x32", w, pos)
        worst = max(worst, w)
    # one-hot dout: dsum is that row's dn exactly
    for r in sorted({0, rows - 1, min(1025, rows - 1)}):
        ch = T.bn_swish_bwd_case(rows, C, onehot=r)
        dn, dsum = run_bn_swish_bwd(L, ch, stage1_only=True, scalar=scalar)[:2]
        assert torch.equal(dsum[:C], dn[r]) and float(dn[torch.arange(rows) != r].abs().sum()) == 0.0, r
    report("bn_swish_bwd C %d rows %d%s (dn, dsum, d_gamma, d_beta, dz)" % (C, rows, " scalar kernel" if scalar else ""), worst, [])


def run_convmid_bwd(L, c, x32, partials=False, bn=None):
    """ma_convmid_bwd_bf16 / _x32, or with bn = (dn, z, stats, gamma, dsum) ma_convmid_bwd_bn_bf16 -> (dy, d_dw_w, d_dw_b) (the
    accumulated buffers minus what they held, or with partials the float64 sums of the partial vectors), after the guard checks."""
    B, Tn, C, ks = c["B"], c["T"], c["C"], c["ks"]
    dt = torch.float32 if x32 else torch.bfloat16
    y = Guard(B * Tn, 2 * C, dt, ld=2 * C + 8, fill=c["y"])
    dy = Guard(B * Tn, 2 * C, dt, ld=2 * C + 8)
    w = dev(c["w"])
    parts = int(L.ma_convmid_bwd_parts(B, Tn))
    strips = (Tn + 15) // 16
    per_block = 1
    while (strips + per_block - 1) // per_block * B > T.CONV_BWD_MAX_PARTS:
        per_block += 1
    assert parts == (strips + per_block - 1) // per_block * B
    width = C * (ks + 1)
    ws = Guard(parts, width, torch.float32, ld=width, top=1, bottom=1)  # exactly what the launcher asks for
    g = torch.Generator().manual_seed(ks + Tn)
    dw0, db0 = torch.randn(C, ks, generator=g), torch.randn(C, generator=g)
    assert float(dw0.abs().max()) < ACC0_MAX and float(db0.abs().max()) < ACC0_MAX
    dwg, dbg = Guard(C, ks, torch.float32, ld=ks, fill=dw0), vec(C, torch.float32, fill=db0)
    tail = (P(y.view), y.ld, B, Tn, C, P(w), ks, P(dy.view), dy.ld, None if partials else P(dwg.view), None if partials else P(dbg.flat()),
            P(ws.view), parts * width * 4, st())
    if bn is None:
        dz = dev(c["dz"].float())
        rc = (L.ma_convmid_bwd_x32 if x32 else L.ma_convmid_bwd_bf16)(P(dz), *tail)
    else:
        dn, z, stats, gamma, dsum = (dev(t.float()) for t in bn)
        rc = L.ma_convmid_bwd_bn_bf16(P(dn), P(z), P(stats), P(gamma), P(dsum), *tail)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert dy.intact() is None and y.untouched() and ws.intact() is None, (dy.intact(), ws.intact())
    if partials:
        assert dwg.untouched() and dbg.untouched()
        tot = ws.view.double().sum(0).cpu()
        return dy.view.cpu(), tot[:C * ks].view(C, ks), tot[C * ks:]
    assert dwg.intact() is None and dbg.intact() is None
    return dy.view.cpu(), dwg.view.cpu().double() - dw0.double(), dbg.flat().cpu().double() - db0.double()


ACC0_MAX = 6.0  # |randn| of the C * ks + C values a gradient buffer held before the launch stays below this (asserted at the fill)


def _acc(case):
    """The parameter gradients were added into non-zero float32 buffers and the test subtracts what they held: the addition rounds at
    |buffer + sum| <= ACC0_MAX + |sum|, the float64 subtraction not at all."""
    return {"want": case["want"], "bound": case["bound"] + T.U * (case["want"].abs() + ACC0_MAX)}


@pytest.mark.parametrize("ks", T.CONV_KS)
def test_convmid_bwd_routing(L, ks):
    """One-hot dz and one-hot s with power-of-two weights, float32 mode, exact: the reversed-tap footprint cut at the utterance's
    ends, d_dw_w[c][t1 - t0 + pad] the product and every other tap zero, across the strip edge 15 | 16 and across utterances."""
    for Tn in T.CONV_TS:
        for C in ((256, 512) if Tn == 17 else (256,)):
            for i, (t0, t1, b0, b1) in enumerate(T.conv_bwd_routes(Tn)):
                c = T.conv_bwd_route_case(ks, Tn, C, t0, t1, b0, b1)
                dy, dw, db = run_convmid_bwd(L, c, True, partials=True)
                for name, got in (("dy", dy), ("dw", dw.float()), ("db", db.float())):
                    w, pos = T.check_exact(got + 0.0, c[name])
                    assert w == 0, (name, ks, Tn, C, t0, t1, b0, b1, pos)


@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("ks", T.CONV_KS)
def test_convmid_bwd_random(L, ks, x32):
    worst = [0.0, 0.0]
    for Tn in T.CONV_TS:
        for C in ((256, 512) if Tn == 47 else (256,)):
            c = T.conv_bwd_random_case(ks, Tn, C, x32)
            for partials in (False, True):
                dy, dw, db = run_convmid_bwd(L, c, x32, partials=partials)
                w, pos = T.check_conv_dy(dy, c["dy"])
                assert w <= 1 and not pos, ("dy", ks, Tn, C, w, pos)
                worst[0] = max(worst[0], w)
                for name, got in (("dw", dw), ("db", db)):
                    w, pos = T.check_bound(got, c[name] if partials else _acc(c[name]))
                    assert w <= 1 and not pos, (name, ks, Tn, C, partials, w, pos)
                    worst[1] = max(worst[1], w)
    report("convmid_bwd%s ks %d dy%s" % ("_x32" if x32 else "", ks, "" if x32 else " (share != RNE / 0.5 %)"), worst[0], [])
    report("convmid_bwd%s ks %d d_dw_w, d_dw_b" % ("_x32" if x32 else "", ks), worst[1], [])


def test_convmid_bwd_per_block_2(L):
    """B = 700, T = 33: three strips x 700 > 2048 partial vectors, so a workgroup walks two strips and the second workgroup of every
    utterance finds its second strip past T."""
    B, Tn, C, ks = 700, 33, 256, 3
    assert int(L.ma_convmid_bwd_parts(B, Tn)) == 2 * B
    c = T.conv_bwd_random_case(ks, Tn, C, False, B=B)
    dy, dw, db = run_convmid_bwd(L, c, False, partials=True)  # (asserts that exactly ma_convmid_bwd_parts vectors are filled)
    worst = 0.0
    for got, case, chk in ((dy, c["dy"], T.check_conv_dy), (dw, c["dw"], T.check_bound), (db, c["db"], T.check_bound)):
        w, pos = chk(got, case)
        assert w <= 1 and not pos, (w, pos)
        worst = max(worst, w)
    report("convmid_bwd per_block = 2 (B 700, T 33)", worst, [])


@pytest.mark.parametrize("ks,Tn", ((15, 47), (3, 17), (31, 5)))
def test_convmid_bwd_fused_bn(L, ks, Tn):
    """Stage 1 + ma_convmid_bwd_bn_bf16 (the BatchNorm backward's second stage inside the depthwise backward's loads) against float64:
    dz's own bound passes through the taps."""
    B, C = 3, 256
    cb = T.bn_swish_bwd_case(B * Tn, C)
    dn, dsum = run_bn_swish_bwd(L, cb, stage1_only=True)[:2]
    c = T.conv_bwd_random_case(ks, Tn, C, False, B=B, dz=cb["dz"]["want"], dz_bound=cb["dz"]["bound"])
    dy, dw, db = run_convmid_bwd(L, c, False, partials=True, bn=(dn, cb["z"], cb["stats"], cb["gamma"], dsum))
    w, pos = T.check_conv_dy(dy, c["dy"])
    assert w <= 1 and not pos, ("dy", w, pos)
    for name, got in (("dw", dw), ("db", db)):  # the parameter gradients of the fused form, from the dz it made on the fly
        w2, pos = T.check_bound(got, c[name])
        assert w2 <= 1 and not pos, (name, w2, pos)
    report("convmid_bwd_bn ks %d T %d dy (share != RNE / 0.5 %%)" % (ks, Tn), w, [])


# ---- subsampling backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x32", (False, True))
def test_relu_bwd(L, x32):
    c = T.relu_bwd_case(x32=x32)
    dy = vec(c["n"], c["dy"].dtype, fill=c["dy"])
    y = dev(c["y"])
    rc = (L.ma_relu_bwd_x32 if x32 else L.ma_relu_bwd_bf16)(P(dy.flat()), P(y), c["n"], st())
    torch.cuda.synchronize()
    assert rc == 0 and dy.intact() is None
    w, pos = T.check_exact(dy.flat().cpu(), c)
    assert w == 0, pos


@pytest.mark.parametrize("shape", T.SUB_SHAPES)
def test_im2col_t(L, shape):
    c = T.subsample_case(shape)
    b, h, w, ch = shape
    m = c["m"]
    ld = (m + 63) // 64 * 64
    out = Guard(9 * ch, ld, torch.bfloat16, ld=ld + 8)  # the window includes the pad columns m .. ld - 1: they stay as the caller left them
    act = dev(c["act"])
    rc = L.ma_im2col_t_3x3s2_nhwc_bf16(P(act), b, h, w, ch, P(out.view), out.ld, st())
    torch.cuda.synchronize()
    assert rc == 0 and out.intact(owned=False) is None, out.intact(owned=False)
    got = out.view.cpu()
    assert T.check_exact(got[:, :m].contiguous(), c["im2col"])[0] == 0, T.check_exact(got[:, :m].contiguous(), c["im2col"])[1]
    assert bool((bits(got[:, m:]) == BF16_SENTINEL).all())


@pytest.mark.parametrize("x32", (False, True))
@pytest.mark.parametrize("shape", T.SUB_SHAPES)
def test_col2im_relu(L, shape, x32):
    c = T.subsample_case(shape, x32)
    b, h, w, ch = shape
    out = Guard(b * h * w, ch, c["act"].dtype, ld=ch)
    fn = L.ma_col2im_3x3s2_relu_x32 if x32 else L.ma_col2im_3x3s2_relu_bf16
    dcol, act = dev(c["dcol"]), dev(c["act"])
    rc = fn(P(dcol), P(act), b, h, w, ch, P(out.view), st())
    torch.cuda.synchronize()
    assert rc == 0 and out.intact() is None, out.intact()
    got = out.view.cpu().view(b, h, w, ch)
    w_, pos = T.check_exact(got, c["col2im"])
    assert w_ == 0, pos
    if h % 2 == 0:
        assert float(got[:, h - 1].float().abs().max()) == 0.0
    if w % 2 == 0:
        assert float(got[:, :, w - 1].float().abs().max()) == 0.0


@pytest.mark.parametrize("shape", T.CONV1_SHAPES)
def test_conv1_dw(L, shape):
    """ma_subsample_conv1_dw_f32 / _x32 through the three kernels its launcher picks (8 channels with LDS staging, 8 channels without,
    scalar at C = 260): integer dact and x give exact dw / db (added into integer buffers); with CMVN a derived per-element bound."""
    b, t, idim, ch = shape
    nbytes = int(L.ma_train_reduce_workspace_bytes())
    ws = torch.empty(nbytes // 4, device="cuda")
    worst = 0.0
    for x32 in (False, True):
        for cmvn in (False, True):
            c = T.conv1_dw_case(shape, x32, cmvn)
            dact, x = dev(c["dact"]), dev(c["x"])
            mean, istd = dev(c["mean"]), dev(c["istd"])
            dw, db = Guard(ch, 9, torch.float32, ld=9, fill=c["dw0"]), vec(ch, torch.float32, fill=c["db0"])
            fn = L.ma_subsample_conv1_dw_x32 if x32 else L.ma_subsample_conv1_dw_f32
            rc = fn(P(dact), P(x), b, t, idim, P(mean), P(istd), ch, P(dw.view), P(db.flat()), P(ws), nbytes, st())
            torch.cuda.synchronize()
            assert rc == 0 and dw.intact() is None and db.intact() is None, (rc, dw.intact(), db.intact())
            w, pos = T.check_conv1_dw((dw.view, db.flat()), c)
            assert w <= 1 and not pos, (shape, x32, cmvn, w, pos)
            worst = max(worst, w)
    report("conv1_dw B %d T %d idim %d C %d (exact without CMVN)" % shape, worst, [])


# ---- optimizer ---------------------------------------------------------------------------------------------------------------------
def test_grad_overflow(L):
    n = T.OVERFLOW_N  # 2048 workgroups x 256 threads + 3: the last three indices are reached by the wrapped loop only
    base = torch.randn(n, generator=torch.Generator().manual_seed(1))
    base[5], base[6], base[7] = torch.finfo(torch.float32).max, 2.0 ** -149, -2.0 ** -130
    g = base.cuda()
    flag = vec(1, torch.int32, fill=torch.zeros(1, dtype=torch.int32))

    def run(expect, start=0):
        flag.flat().fill_(start)
        assert L.ma_grad_overflow_f32(P(g), n, P(flag.flat()), st()) == 0
        torch.cuda.synchronize()
        assert flag.intact(owned=False) is None and int(flag.flat()[0]) == expect

    run(0)
    run(1, start=1)  # a flag already 1 stays 1
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i in (0, n - 1, 2048 * 256 + 1):
            g[i] = bad
            run(T.overflow_ref(g.cpu()))
            assert T.overflow_ref(g.cpu()) == 1
            g[i] = base[i]
    run(0)
    one = torch.tensor([float("nan")]).cuda()
    assert L.ma_grad_overflow_f32(P(one), 1, P(flag.flat()), st()) == 0 and int(flag.flat()[0]) == 1


def run_adam(L, c, mirror):
    n = c["n"]
    p, m, v = (vec(n, torch.float32, fill=c[k]) for k in ("p", "m", "v"))
    g = dev(c["g"])
    ov = torch.tensor([c["overflow"]], dtype=torch.int32).cuda()
    hp = c["hp"]
    a = (hp["lr_t"], hp["beta1"], hp["beta2"], hp["eps"], hp["inv_scale"])
    if mirror:
        c["mirror0"] = T.bf16_rne(c["p"])
        mir = vec(n, torch.bfloat16, fill=c["mirror0"] if c["overflow"] else None)
        rc = L.ma_adam_mirror_f32(P(p.flat()), P(g), P(m.flat()), P(v.flat()), n, *a, P(ov), P(mir.flat()), st())
    else:
        rc = L.ma_adam_f32(P(p.flat()), P(g), P(m.flat()), P(v.flat()), n, *a, P(ov), st())
    torch.cuda.synchronize()
    assert rc == 0
    outs = (p, m, v) + ((mir,) if mirror else ())
    for gd in outs:
        assert gd.intact() is None, gd.intact()
        if c["overflow"]:
            assert gd.untouched()
    return tuple(gd.flat().cpu() for gd in outs)


# 1 048 580 wraps adam_kernel's loop (4096 x 256 < n); the mirror kernel walks quads and wraps from 4 x 4096 x 256 on: 4 194 308
@pytest.mark.parametrize("n", (1, 4, 1048580, 4194308))
def test_adam_and_mirror(L, n):
    for overflow in (0, 1):
        c = T.adam_case(n, overflow=overflow)
        plain = run_adam(L, c, False)
        w, pos = T.check_adam(plain, c)
        assert w <= 1 and not pos, (overflow, w, pos)
        if n % 4 == 0:
            mir = run_adam(L, c, True)
            w2, pos = T.check_adam(mir, c)
            assert w2 <= 1 and not pos, (overflow, w2, pos)
            for a, b in zip(plain, mir):
                assert torch.equal(bits(a), bits(b))  # the same p, m, v bit for bit
            w = max(w, w2)
        if not overflow:
            assert bool(torch.isfinite(plain[0]).all()) and float(plain[0][0]) == float(c["p"][0])  # v = g = m = 0: a step of 0
            report("adam n %d (p, m, v; mirror exact)" % n, w, [])


def test_adam_mirror_ties(L):
    c = T.adam_case(64, lr_t=0.0)
    got = run_adam(L, c, True)
    assert torch.equal(bits(got[0]), bits(c["p"]))  # lr_t = 0: the new p is p, exactly halfway between two bf16 numbers
    w, pos = T.check_adam(got, c)
    assert w <= 1 and not pos, pos


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """What the launchers refuse by their own checks: the documented code, nothing written."""
    from mindaudio_amd import _lib

    INV, UNS, WS = _lib.MA_ERR_INVALID_ARG, _lib.MA_ERR_UNSUPPORTED, _lib.MA_ERR_WORKSPACE
    s = st()
    rows = 5
    # LayerNorm backward: a width outside the four, a workspace one byte short
    for D, nbytes, want in ((320, 1 << 20, UNS), (128, 1 << 20, UNS), (256, 2 * 2 * 256 * 4 - 1, WS), (512, 2 * 2 * 512 * 4 - 1, WS)):
        x, g = Guard(rows, D, torch.float32, ld=D + 4), Guard(rows, D, torch.float32, ld=D + 4)
        dg, db, ws = vec(D, torch.float32), vec(D, torch.float32), vec(1 << 18, torch.float32)
        dy, gamma = torch.zeros(rows, D, device="cuda"), torch.ones(D, device="cuda")
        rc = L.ma_layernorm_bwd_f32(P(x.view), x.ld, rows, D, P(gamma), 1e-5, None, P(dy), D, 0, P(g.view), g.ld, 1, P(dg.flat()),
                                    P(db.flat()), P(ws.flat()), nbytes, s)
        torch.cuda.synchronize()
        assert rc == want and all(t.untouched() for t in (x, g, dg, db, ws)), (D, rc)
        if D == 256:
            dyn = Guard(rows, 256, torch.bfloat16, ld=264)
            for p, ldn, nb, want2 in ((0.1, 264, nbytes, WS), (1.0, 264, 1 << 20, UNS), (0.1, 252, 1 << 20, UNS)):
                rc = L.ma_layernorm_bwd_next_f32(P(x.view), x.ld, rows, D, P(gamma), 1e-5, None, P(dy), D, 0, P(g.view), g.ld, 1,
                                                 P(dg.flat()), P(db.flat()), P(ws.flat()), nb, P(dyn.view), ldn, 0.5, None, p, 1, 2, s)
                torch.cuda.synchronize()
                assert rc == want2 and all(t.untouched() for t in (x, g, dg, db, ws, dyn)), (p, ldn, rc)
    # act_dropout bf16: n % 8 != 0; p >= 1 everywhere
    u = torch.ones(1328, dtype=torch.bfloat16, device="cuda")
    uf = torch.ones(1328, device="cuda")
    h, hf = vec(1328, torch.bfloat16), vec(1328, torch.float32)
    for n, p, want in ((1321, 0.1, UNS), (1320, 1.0, INV), (1320, 1.5, INV)):
        for act in (T.ACT_SWISH, T.ACT_RELU):
            assert L.ma_act_dropout_fwd_bf16(P(u), P(h.flat()), n, act, p, 1, 2, s) == want
            assert L.ma_act_dropout_bwd_bf16(P(u), P(u), P(h.flat()), n, act, p, 1, 2, s) == want
            if want == INV:
                assert L.ma_act_dropout_fwd_x32(P(uf), P(hf.flat()), n, act, p, 1, 2, s) == INV
                assert L.ma_act_dropout_bwd_x32(P(uf), P(uf), P(hf.flat()), n, act, p, 1, 2, s) == INV
    torch.cuda.synchronize()
    assert h.untouched() and hf.untouched()
    # dropout_add / dropout_bwd: ld < cols on each operand, p >= 1
    cols = 264
    out, xin = Guard(rows, cols, torch.float32, ld=cols + 8), Guard(rows, cols, torch.float32, ld=cols + 8)
    dyb, dyf = Guard(rows, cols, torch.bfloat16, ld=cols + 8), Guard(rows, cols, torch.float32, ld=cols + 8)
    y = torch.ones(rows, cols, device="cuda")
    for ldo, ldx, ldy, p in ((cols - 8, cols + 8, cols, 0.1), (cols + 8, cols - 8, cols, 0.1), (cols + 8, cols + 8, cols - 8, 0.1),
                             (cols + 8, cols + 8, cols, 1.0)):
        assert L.ma_dropout_add_f32(P(out.view), ldo, P(xin.view), ldx, P(y), ldy, 0, rows, cols, 0.5, p, 1, 2, s) == INV
    for ldg, ldd, p in ((cols - 8, cols + 8, 0.1), (cols, cols - 8, 0.1), (cols, cols + 8, 1.0)):
        assert L.ma_dropout_bwd_bf16(P(y), ldg, P(dyb.view), ldd, rows, cols, 0.5, None, p, 1, 2, s) == INV
        assert L.ma_dropout_bwd_x32(P(y), ldg, P(dyf.view), ldd, rows, cols, 0.5, None, p, 1, 2, s) == INV
    torch.cuda.synchronize()
    assert all(t.untouched() for t in (out, xin, dyb, dyf))
    # bf16 col2im: C % 8 != 0; im2col_t: ld_out < M
    b, hh, ww, ch = 2, 5, 5, 12
    act = torch.ones(b, hh, ww, ch, dtype=torch.bfloat16, device="cuda")
    dcol = torch.ones(b * 4, 9 * ch, dtype=torch.bfloat16, device="cuda")
    dact = Guard(b * hh * ww, ch, torch.bfloat16, ld=ch)
    assert L.ma_col2im_3x3s2_relu_bf16(P(dcol), P(act), b, hh, ww, ch, P(dact.view), s) == UNS
    colt = Guard(9 * ch, 64, torch.bfloat16, ld=64)
    assert L.ma_im2col_t_3x3s2_nhwc_bf16(P(act), b, hh, ww, ch, P(colt.view), b * 4 - 1, s) == INV
    torch.cuda.synchronize()
    assert dact.untouched() and colt.untouched()
    # conv-module forward: ks outside {3, 7, 15, 31}, C % 256 != 0
    yb = torch.zeros(6, 2 * 320, dtype=torch.bfloat16, device="cuda")
    wz, bz = torch.zeros(320, 31, device="cuda"), torch.zeros(320, device="cuda")
    zg, sg = Guard(6, 320, torch.float32, ld=320), Guard(3, 640, torch.float32, ld=640)
    for C_, ks_ in ((256, 5), (256, 1), (256, 33), (320, 15), (128, 15)):
        assert L.ma_convmid_fwd_train(P(yb), 2 * C_, 3, 2, C_, P(wz), ks_, P(bz), P(zg.view), P(sg.view), s) == UNS
        assert L.ma_convmid_fwd_train_x32(P(yb), 2 * C_, 3, 2, C_, P(wz), ks_, P(bz), P(zg.view), P(sg.view), s) == UNS
    torch.cuda.synchronize()
    assert zg.untouched() and sg.untouched()
    # conv-module backward: ks, C % 256, a workspace one byte short
    dzz, dyg = torch.zeros(6, 320, device="cuda"), Guard(6, 640, torch.bfloat16, ld=648)
    wsg = vec(2 * 256 * 16, torch.float32)
    for C_, ks_, nb, want in ((256, 5, 1 << 20, UNS), (320, 15, 1 << 20, UNS), (256, 15, 3 * 256 * 16 * 4 - 1, WS)):
        assert L.ma_convmid_bwd_bf16(P(dzz), P(yb), 2 * C_, 3, 2, C_, P(wz), ks_, P(dyg.view), dyg.ld, None, None, P(wsg.flat()), nb, s) == want
    bws = vec(16, torch.float32)
    assert L.ma_bn_swish_bwd_f32(P(yb), P(dzz), P(wz), P(bz), P(bz), P(zg.view), 6, 256, P(sg.view), None, None, P(bws.flat()),
                                 T.BN_BWD_BLOCKS * 2 * 256 * 4 - 1, s) == WS
    torch.cuda.synchronize()
    assert dyg.untouched() and wsg.untouched() and bws.untouched() and zg.untouched() and sg.untouched()
    # the mirror: n % 4 != 0 is answered with UNSUPPORTED (the caller keeps adam + cast) and nothing is touched
    n = 1001
    p_, m_, v_ = (vec(n, torch.float32, fill=torch.ones(n)) for _ in range(3))
    mir = vec(n, torch.bfloat16)
    gr = torch.ones(n, device="cuda")
    assert L.ma_adam_mirror_f32(P(p_.flat()), P(gr), P(m_.flat()), P(v_.flat()), n, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, P(mir.flat()), s) == UNS
    torch.cuda.synchronize()
    assert all(t.untouched() for t in (p_, m_, v_, mir))
