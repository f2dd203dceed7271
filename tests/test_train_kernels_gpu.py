"""GPU parity of the training-step kernels (mindaudio_amd/csrc/train_kernels.hip) against float32 PyTorch-CPU
restatements of the same formulas (autograd of the oracle's layer definitions).

The attention backward kernels are also checked ROW BY ROW (test_attention_backward_rows, test_decoder_attention_backward_rows; inputs,
float64 references and the rounded models in tests/attention_cases.py): worst row error ||got_i - ref_i|| / max(||ref_i||, floor)
against float64 autograd, measured on an MI355X, as  bf16 kernel / rounded reference / float32 kernel.  The bf16 kernel must stay within
4 x the rounded reference, the float32 kernel within 2e-5.

  b3 t1 h4 pad          dq 1.52e-4 / 2.30e-4 / 0   dk 1.55e-4 / 2.25e-4 / 0   dv 0 / 0 / 0
                        dpos 2.03e-4 / 2.43e-4 / 0   du 1.82e-4 / 2.24e-4 / 0   dbv 1.20e-4 / 1.00e-4 / 0
  b3 t1 h4 chunk        dq 7.81e-5 / 5.25e-5 / 0   dk 6.86e-5 / 5.24e-5 / 0   dv 0 / 0 / 0
                        dpos 8.65e-5 / 5.75e-5 / 0   du 8.39e-5 / 5.04e-5 / 0   dbv 4.67e-5 / 2.56e-5 / 0
  b3 t17 h4 pad         dq 7.40e-3 / 8.01e-3 / 1.06e-6   dk 8.23e-3 / 7.75e-3 / 7.17e-7   dv 5.04e-3 / 5.04e-3 / 6.71e-7
                        dpos 7.85e-3 / 7.62e-3 / 7.51e-7   du 3.78e-3 / 3.85e-3 / 5.48e-7   dbv 3.44e-3 / 3.58e-3 / 5.37e-7
  b3 t17 h4 chunk       dq 8.84e-3 / 9.20e-3 / 1.21e-6   dk 1.11e-2 / 1.17e-2 / 1.12e-6   dv 5.25e-3 / 5.25e-3 / 1.10e-6
                        dpos 1.10e-2 / 1.16e-2 / 1.11e-6   du 5.34e-3 / 5.97e-3 / 6.79e-7   dbv 5.66e-3 / 6.16e-3 / 6.70e-7
  b3 t65 h4 pad         dq 3.03e-2 / 2.96e-2 / 2.06e-6   dk 7.88e-3 / 7.63e-3 / 1.66e-6   dv 7.40e-3 / 7.40e-3 / 1.34e-6
                        dpos 6.95e-3 / 6.48e-3 / 1.73e-6   du 3.88e-3 / 3.67e-3 / 6.65e-7   dbv 4.06e-3 / 3.64e-3 / 6.78e-7
  b3 t65 h4 chunk       dq 1.73e-2 / 1.37e-2 / 1.67e-6   dk 1.90e-2 / 2.85e-2 / 2.16e-6   dv 9.00e-3 / 8.30e-3 / 1.59e-6
                        dpos 8.77e-3 / 7.73e-3 / 1.48e-6   du 3.83e-3 / 3.81e-3 / 6.80e-7   dbv 4.14e-3 / 4.05e-3 / 6.83e-7
  b3 t97 h4 pad         dq 1.27e-2 / 1.04e-2 / 1.93e-6   dk 1.34e-2 / 1.11e-2 / 1.88e-6   dv 7.73e-3 / 7.73e-3 / 1.66e-6
                        dpos 7.03e-3 / 6.72e-3 / 2.04e-6   du 3.90e-3 / 3.84e-3 / 9.03e-7   dbv 4.03e-3 / 4.03e-3 / 7.92e-7
  b3 t97 h4 chunk       dq 1.85e-2 / 1.88e-2 / 2.82e-6   dk 1.36e-2 / 1.06e-2 / 1.86e-6   dv 8.74e-3 / 8.77e-3 / 1.97e-6
                        dpos 7.50e-3 / 6.85e-3 / 1.22e-6   du 3.95e-3 / 3.81e-3 / 6.83e-7   dbv 3.73e-3 / 3.65e-3 / 7.44e-7
  b2 t129 h4 pad        dq 2.31e-2 / 2.31e-2 / 2.00e-6   dk 8.74e-3 / 8.68e-3 / 1.63e-6   dv 7.52e-3 / 7.52e-3 / 1.85e-6
                        dpos 8.96e-3 / 8.90e-3 / 1.68e-6   du 3.94e-3 / 3.83e-3 / 8.68e-7   dbv 3.84e-3 / 3.83e-3 / 9.15e-7
  b2 t129 h4 chunk      dq 3.77e-2 / 4.22e-2 / 3.13e-6   dk 5.57e-2 / 5.93e-2 / 2.43e-6   dv 1.12e-2 / 1.12e-2 / 2.81e-6
                        dpos 7.91e-3 / 8.07e-3 / 1.12e-6   du 4.03e-3 / 4.01e-3 / 6.57e-7   dbv 3.90e-3 / 3.97e-3 / 6.82e-7
  b2 t65 h8 pad         dq 9.65e-3 / 9.89e-3 / 1.23e-6   dk 6.87e-3 / 7.61e-3 / 1.34e-6   dv 5.90e-3 / 5.90e-3 / 1.11e-6
                        dpos 7.01e-3 / 7.40e-3 / 1.20e-6   du 4.23e-3 / 4.17e-3 / 7.38e-7   dbv 4.18e-3 / 4.29e-3 / 7.04e-7
  b2 t65 h8 chunk       dq 1.01e-2 / 9.62e-3 / 1.45e-6   dk 2.22e-2 / 2.03e-2 / 1.43e-6   dv 7.64e-3 / 7.60e-3 / 1.37e-6
                        dpos 6.52e-3 / 6.69e-3 / 1.30e-6   du 4.58e-3 / 4.42e-3 / 6.05e-7   dbv 4.43e-3 / 4.45e-3 / 6.51e-7
  lq1 lk1 mode0         dq 6.36e-5 / 6.36e-5 / 0   dk 7.26e-6 / 7.14e-6 / 0   dv 0 / 0 / 0
  lq33 lk320 mode1      dq 3.40e-3 / 3.40e-3 / 4.43e-7   dk 3.97e-3 / 3.73e-3 / 2.95e-7   dv 4.39e-3 / 3.47e-3 / 2.67e-7
  lq65 lk321 mode1      dq 1.93e-3 / 1.93e-3 / 4.47e-7   dk 3.40e-3 / 1.95e-3 / 3.13e-7   dv 4.28e-3 / 1.95e-3 / 2.45e-7
  lq64 lk64 mode2       dq 7.25e-3 / 7.25e-3 / 2.90e-7   dk 5.25e-3 / 5.04e-3 / 2.23e-7   dv 3.38e-3 / 3.38e-3 / 1.88e-7
  lq97 lk97 mode2       dq 6.26e-3 / 6.26e-3 / 3.76e-7   dk 4.94e-3 / 3.93e-3 / 3.18e-7   dv 4.77e-3 / 3.56e-3 / 1.95e-7
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    from mindaudio_amd.train import kernels

    return kernels


def bf(x):
    return x.to(torch.bfloat16)


def rel(got, want):
    return float((got.float().cpu() - want).norm() / (want.norm() + 1e-30))


def test_transpose_and_colsum(K):
    g = torch.Generator().manual_seed(0)
    for rows, cols in ((130, 72), (64, 64), (1000, 4233), (7, 256)):
        x = bf(torch.randn(rows, cols, generator=g))
        cs = torch.zeros(cols, device="cuda")
        out = K.transpose(x.cuda(), colsum=cs)
        assert out.shape == (cols, K.pad64(rows))
        assert torch.equal(out[:, :rows].cpu(), x.t())
        assert float(out[:, rows:].abs().sum()) == 0.0
        assert rel(cs, x.float().sum(0)) < 1e-5


def test_transpose_batch_and_batched_split_sums(K):
    """The one-launch forms the training step uses: ma_transpose_batch_bf16 (a list of matrices, bit-exact copies) and
    ma_gemm_tn_partial_bf16 + ma_reduce_splits_batch_f32 (split-K partials of several products, summed by one launch) against
    the per-matrix entry points."""
    import ctypes

    from mindaudio_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    st = torch.cuda.current_stream().cuda_stream

    def to_dev(items, ctype):
        raw = (ctype * len(items))(*items)
        return torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).cuda()

    # ---- transposes ----
    shapes = ((256, 2048), (768, 256), (4240, 256), (72, 136))
    xs = [bf(torch.randn(r, c, generator=g)).cuda() for r, c in shapes]
    outs = [torch.zeros((c, K.pad64(r)), dtype=torch.bfloat16, device="cuda") for r, c in shapes]
    items, block_item, first = [], [], 0
    for i, (x, o) in enumerate(zip(xs, outs)):
        r, c = x.shape
        tr, tc = (r + 63) // 64, (c + 63) // 64
        items.append(_lib.TransposeItem(x.data_ptr(), o.data_ptr(), x.stride(0), o.stride(0), r, c, first, tc))
        block_item += [i] * (tr * tc)
        first += tr * tc
    d_items, d_map = to_dev(items, _lib.TransposeItem), torch.tensor(block_item, dtype=torch.int32, device="cuda")
    _lib.check(lib.ma_transpose_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), first, st), "tb")
    for x, o in zip(xs, outs):
        assert torch.equal(o[:, :x.shape[0]], x.t()) and float(o[:, x.shape[0]:].abs().sum()) == 0.0
    # ---- split-K products: partials of two weight-gradient shapes, one reduction launch ----
    kc = 3000
    probs = ((512, 256), (256, 768))
    arena, items, block_item, first, want, gouts = [], [], [], 0, [], []
    for i, (mo, no) in enumerate(probs):
        a, b = bf(torch.randn(kc, mo, generator=g)).cuda(), bf(torch.randn(kc, no, generator=g)).cuda()
        nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, kc))
        splits = int(lib.ma_gemm_tn_splits(mo, no, kc))
        assert nbytes == splits * mo * (no + 1) * 4
        part = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        K.gemm_tn_partial(a, b, part, with_colsum=True)
        base, cbase = torch.randn(mo, no, generator=g).cuda(), torch.randn(mo, generator=g).cuda()
        ref, cref = base.clone(), cbase.clone()
        K.gemm_tn(a, b, ref, alpha=0.5, accumulate=True, colsum=cref)
        out, cout = base.clone(), cbase.clone()
        nblk = (mo * no + 1023) // 1024
        items.append(_lib.ReduceItem(part.data_ptr(), out.data_ptr(), mo * no, out.stride(0), no, splits, 0.5, 1, first, 0))
        block_item += [len(items) - 1] * nblk
        first += nblk
        # the bias gradient: one partial column-sum vector per split, behind the partial products
        items.append(_lib.ReduceItem(part.data_ptr() + splits * mo * no * 4, cout.data_ptr(), mo, mo, mo, splits, 1.0, 1, first, 0))
        block_item += [len(items) - 1]
        first += 1
        arena.append(part); want += [ref, cref]; gouts += [out, cout]
        assert rel(cref - cbase, a.float().cpu().sum(0)) < 1e-5
    # a "tall" item (accumulate bit 1): 300 per-workgroup partials of a (dgamma | dbeta) pair, row stride 512
    parts = torch.randn(300, 512, generator=g).cuda()
    tall_out = torch.zeros(512, device="cuda")
    items.append(_lib.ReduceItem(parts.data_ptr(), tall_out.data_ptr(), 512, 512, 512, 300, 1.0, 2, first, 512))
    block_item += [len(items) - 1] * 32
    first += 32
    d_items, d_map = to_dev(items, _lib.ReduceItem), torch.tensor(block_item, dtype=torch.int32, device="cuda")
    _lib.check(lib.ma_reduce_splits_batch_f32(d_items.data_ptr(), d_map.data_ptr(), first, st), "rb")
    for out, ref in zip(gouts, want):
        assert torch.equal(out, ref)  # same partials, same order of the splits
    assert rel(tall_out, parts.double().sum(0).float().cpu()) < 1e-6
    tall_again = torch.zeros(512, device="cuda")
    items[-1] = _lib.ReduceItem(parts.data_ptr(), tall_again.data_ptr(), 512, 512, 512, 300, 1.0, 2, first - 32, 512)
    d_items = to_dev(items, _lib.ReduceItem)
    _lib.check(lib.ma_reduce_splits_batch_f32(d_items.data_ptr(), d_map.data_ptr(), first, st), "rb")
    assert torch.equal(tall_out, tall_again)  # fixed summation order: bit-identical from run to run


def test_partial_group_bad_ninth_item_leaves_first_group_issued(K):
    """ma_gemm_tn_partial_group_bf16 checks and launches per group of eight: a ninth item whose buffer is one byte short is answered
    with MA_ERR_WORKSPACE after the first eight products have been issued (their partials are those of the single-product entry
    point, bit for bit) and before anything of the second group is."""
    from mindaudio_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    kc, mo, no = 130, 64, 72
    nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, kc))
    ops = [(bf(torch.randn(kc, mo, generator=g)).cuda(), bf(torch.randn(kc, no, generator=g)).cuda()) for _ in range(9)]
    parts = [torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(9)]
    items = (_lib.TnItem * 9)()
    for it, (a, b), part in zip(items, ops, parts):
        it.A, it.B, it.partial, it.lda, it.ldb = a.data_ptr(), b.data_ptr(), part.data_ptr(), a.stride(0), b.stride(0)
        it.Mo, it.No, it.Kc, it.Mo_store, it.partial_bytes, it.with_colsum = mo, no, kc, mo, nbytes, 1
    items[8].partial_bytes = nbytes - 1
    assert lib.ma_gemm_tn_partial_group_bf16(items, 9, torch.cuda.current_stream().cuda_stream) == _lib.MA_ERR_WORKSPACE
    for (a, b), part in zip(ops[:8], parts[:8]):
        alone = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        K.gemm_tn_partial(a, b, alone, with_colsum=True)
        assert torch.equal(part, alone)
    assert bool((parts[8] == 0x5A).all())


def test_gemm_splitk(K):
    g = torch.Generator().manual_seed(1)
    for m, n, k in ((256, 256, 10240), (2048, 256, 4096), (100, 300, 640), (256, 2304, 64 * 300)):
        a, w = bf(torch.randn(m, k, generator=g)), bf(torch.randn(n, k, generator=g))
        out = torch.zeros(m, n, device="cuda")
        K.gemm_splitk(a.cuda(), w.cuda(), out, alpha=0.5)
        want = 0.5 * (a.float() @ w.float().t())
        assert rel(out, want) < 2e-5


def test_layernorm_bwd(K):
    from mindaudio_amd import ops

    g = torch.Generator().manual_seed(2)
    rows = 1001
    x = (torch.randn(rows, 256, generator=g) * 2 + 0.3).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(256, generator=g)).requires_grad_()
    beta = (0.1 * torch.randn(256, generator=g)).requires_grad_()
    rs = (torch.rand(rows, generator=g) > 0.2).float()
    dy = torch.randn(rows, 256, generator=g)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = ((x - mu) / torch.sqrt(var + 1e-5) * gamma + beta) * rs[:, None]
    y.backward(dy)
    for dy_dev in (dy.cuda(), bf(dy).cuda()):
        g0 = torch.randn(rows, 256, generator=g)
        gbuf = g0.clone().cuda()
        dg, db = torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")
        K.layernorm_bwd(x.detach().cuda(), gamma.detach().cuda(), dy_dev, gbuf, dg, db, row_scale=rs.cuda())
        tol = 1e-5 if dy_dev.dtype == torch.float32 else 4e-3
        assert rel(gbuf, g0 + x.grad) < tol
        assert rel(dg, gamma.grad) < tol and rel(db, beta.grad) < tol
    # in place (dy is g itself, no accumulation)
    gbuf = dy.clone().cuda()
    K.layernorm_bwd(x.detach().cuda(), gamma.detach().cuda(), gbuf, gbuf, torch.zeros(256, device="cuda"),
                    torch.zeros(256, device="cuda"), row_scale=rs.cuda(), accumulate=False)
    assert rel(gbuf, x.grad) < 1e-5


def test_act_dropout_and_dropout_add(K):
    g = torch.Generator().manual_seed(3)
    u = bf(torch.randn(300, 2048, generator=g) * 2)
    for p in (0.0, 0.1):
        h = K.act_dropout_fwd(u.cuda(), p, 77, 5).float().cpu()
        sw = u.float() * torch.sigmoid(u.float())
        keep = (h != 0) | (sw.abs() < 1e-30)
        if p == 0.0:
            assert rel(h, bf(sw).float()) < 1e-3  # v_rcp_f32 in the sigmoid: a few values flip one bf16 ulp at a rounding boundary
        else:
            frac = 1.0 - keep.float().mean().item()
            assert abs(frac - p) < 0.01
            assert rel(h[keep], bf(sw / (1 - p)).float()[keep]) < 4e-3
        dh = bf(torch.randn(300, 2048, generator=g))
        du = K.act_dropout_bwd(u.cuda(), dh.cuda(), p, 77, 5).float().cpu()
        s = torch.sigmoid(u.float())
        want = dh.float() * (s + u.float() * s * (1 - s)) * keep.float() / (1 - p)
        assert rel(du, want) < 4e-3
        # same (seed, salt) -> same mask; a different salt decorrelates
        h2 = K.act_dropout_fwd(u.cuda(), p, 77, 6).float().cpu()
        if p > 0:
            assert ((h2 != 0) != (h != 0)).float().mean() > 0.1
    x = torch.randn(257, 256, generator=g)
    y = torch.randn(257, 256, generator=g)
    for yy in (y, bf(y)):
        xd = K.dropout_add(x.cuda(), yy.cuda(), 0.5, 0.1, 9, 3)
        delta = (xd.cpu() - x) / 0.5
        keep = delta != 0
        assert abs(1 - keep.float().mean().item() - 0.1) < 0.02
        assert rel(delta[keep], (yy.float() / 0.9)[keep]) < 1e-5
        gg = torch.randn(257, 256, generator=g)
        rs = (torch.rand(257, generator=g) > 0.3).float()
        dy = K.dropout_bwd(gg.cuda(), 0.5, 0.1, 9, 3, row_scale=rs.cuda()).float().cpu()
        assert rel(dy, bf(0.5 * gg * keep.float() / 0.9 * rs[:, None]).float()) < 1e-6


# (64, 255): 16 strips x 64 utterances = 1 024 workgroups in the forward and the backward launch (more than three resident rounds)
# c = 512 / 768: the 256-channel slabs of d_model 512 / 768 (round 6: the launches took c = 256 only)
@pytest.mark.parametrize("b,t,c", [(3, 37, 256), (64, 255, 256), (3, 37, 512), (5, 70, 768), (20, 255, 1024)])
def test_convmid_train_fwd_bwd(K, b, t, c):
    g = torch.Generator().manual_seed(4)
    ks = 15
    y = bf(torch.randn(b * t, 2 * c, generator=g))
    dw_w = (0.3 * torch.randn(c, ks, generator=g)).requires_grad_()
    dw_b = (0.1 * torch.randn(c, generator=g)).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).requires_grad_()
    beta = (0.1 * torch.randn(c, generator=g)).requires_grad_()
    yf = y.float().requires_grad_()
    a, gate = yf[:, :c], yf[:, c:]
    s = (a * torch.sigmoid(gate)).view(b, t, c).transpose(1, 2)
    z = F.conv1d(s, dw_w[:, None, :], dw_b, padding=ks // 2, groups=c).transpose(1, 2).reshape(b * t, c)
    bn = torch.nn.BatchNorm1d(c, eps=1e-5, momentum=0.1)
    bn.weight.data, bn.bias.data = gamma.detach().clone(), beta.detach().clone()
    bn.train()
    n = bn(z)
    out = n * torch.sigmoid(n)
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    o_d, z_d, st = K.convmid_fwd_train(y.cuda(), b, t, dw_w.detach().cuda(), dw_b.detach().cuda(), gamma.detach().cuda(),
                                       beta.detach().cuda(), rm, rv)
    assert rel(z_d, z.detach()) < 1e-5
    assert rel(o_d, out.detach()) < 4e-3
    assert rel(rm, bn.running_mean) < 1e-4 and rel(rv, bn.running_var) < 1e-4
    dout = bf(torch.randn(b * t, c, generator=g))
    out.backward(dout.float())
    dws, dbs = torch.zeros(c, ks, device="cuda"), torch.zeros(c, device="cuda")
    dgs, dbe = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dy = K.convmid_bwd(dout.cuda(), y.cuda(), z_d, st, b, t, dw_w.detach().cuda(), gamma.detach().cuda(),
                       beta.detach().cuda(), dws, dbs, dgs, dbe)
    assert rel(dy, yf.grad) < 5e-3
    assert rel(dws, dw_w.grad) < 1e-3
    # the depthwise bias feeds a BatchNorm: its gradient is identically zero (both sides hold rounding noise)
    assert float(dbs.abs().max()) < 1e-3 and float(dw_b.grad.abs().max()) < 1e-3
    assert rel(dgs, bn.weight.grad) < 1e-3 and rel(dbe, bn.bias.grad) < 1e-3
    # the fused step's form (round 4): the BatchNorm backward's second stage inside the depthwise backward's loads, the depthwise
    # partial sums left in the caller's buffer - the same dy up to one float32 rounding, the same parameter gradients
    from mindaudio_amd import _lib
    parts = torch.zeros(int(_lib.load().ma_convmid_bwd_parts(b, t)) * c * (ks + 1), device="cuda")
    dgs2, dbe2 = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dy2 = K.convmid_bwd(dout.cuda(), y.cuda(), z_d, st, b, t, dw_w.detach().cuda(), gamma.detach().cuda(), beta.detach().cuda(), None,
                        None, dgs2, dbe2, partials=parts)
    # the fused form multiplies sum / N before zhat (one rounding apart from bn_bwd2_kernel's order): float32 round-off, then bf16
    assert rel(dy2, dy.float().cpu()) < 1e-3
    assert rel(dgs2, dgs.float().cpu()) < 1e-6 and rel(dbe2, dbe.float().cpu()) < 1e-6
    pv = parts.view(-1, c * (ks + 1)).sum(0)
    assert rel(pv[:c * ks].view(c, ks), dws.cpu()) < 1e-5


def test_subsampling_backward_pieces(K):
    g = torch.Generator().manual_seed(5)
    b, h, w, c = 2, 21, 19, 64
    act = bf(torch.randn(b, h, w, c, generator=g))
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    m = b * ho * wo
    colt = K.im2col_t(act.cuda())
    cols = F.unfold(act.float().permute(0, 3, 1, 2), 3, stride=2)  # (B, C*9, L) with (c, kh, kw) ordering
    cols = cols.view(b, c, 9, ho * wo).permute(2, 1, 0, 3).reshape(9 * c, m)  # -> (khw, c) x (b, ho, wo)
    assert torch.equal(colt[:, :m].cpu().float(), cols)
    dcol = bf(torch.randn(m, 9 * c, generator=g))
    dact = K.col2im_relu(dcol.cuda(), act.cuda()).float().cpu()
    dc = dcol.float().view(b, ho * wo, 9, c).permute(0, 3, 2, 1).reshape(b, c * 9, ho * wo)
    want = F.fold(dc, (h, w), 3, stride=2).permute(0, 2, 3, 1) * (act.float() > 0)
    assert rel(dact, bf(want).float()) < 3e-3
    # conv2 weight gradient as a TN GEMM with the implicit im2col operand
    b2, h2, w2, c2, co2 = 2, 23, 19, 128, 64
    act_b = bf(torch.randn(b2, h2, w2, c2, generator=g))
    ho2, wo2 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    dy_b = bf(torch.randn(b2 * ho2 * wo2, co2, generator=g))
    wgt2 = torch.zeros(co2, c2, 3, 3, requires_grad=True)
    bias2 = torch.zeros(co2, requires_grad=True)
    o2 = F.conv2d(act_b.float().permute(0, 3, 1, 2), wgt2, bias2, stride=2)
    o2.backward(dy_b.float().view(b2, ho2, wo2, co2).permute(0, 3, 1, 2))
    dw2, db2 = torch.zeros(co2, 9 * c2, device="cuda"), torch.zeros(co2, device="cuda")
    K.conv2d_dw(dy_b.cuda(), act_b.cuda(), dw2, db2)
    assert rel(dw2.view(co2, 3, 3, c2), wgt2.grad.permute(0, 2, 3, 1)) < 2e-5 and rel(db2, bias2.grad) < 2e-5
    dy = bf(torch.randn(1000, generator=g)).cuda()
    yv = bf(torch.randn(1000, generator=g))
    assert torch.equal(K.relu_bwd(dy.clone(), yv.cuda()).cpu(), dy.cpu() * (yv.float() > 0).to(torch.bfloat16))
    # conv1 weight gradient (cc = 512 / 1024: slabs of 256 channels, round 6; (40, 255): more partial vectors than one round)
    for bb, tt, idim, cc in ((2, 31, 80, 256), (2, 31, 80, 512), (3, 45, 80, 1024), (40, 255, 80, 512)):
        _conv1_dw_case(K, g, bb, tt, idim, cc)


def _conv1_dw_case(K, g, bb, tt, idim, cc):
    x = torch.randn(bb, tt, idim, generator=g)
    mean, istd = torch.randn(idim, generator=g), 0.5 + torch.rand(idim, generator=g)
    h1, w1 = (tt - 3) // 2 + 1, (idim - 3) // 2 + 1
    dact1 = bf(torch.randn(bb, h1, w1, cc, generator=g))
    wgt = torch.zeros(cc, 1, 3, 3, requires_grad=True)
    bias = torch.zeros(cc, requires_grad=True)
    o = F.conv2d(((x - mean) * istd)[:, None], wgt, bias, stride=2)
    o.backward(dact1.float().permute(0, 3, 1, 2))
    dw, db = torch.zeros(cc, 9, device="cuda"), torch.zeros(cc, device="cuda")
    K.conv1_dw(dact1.cuda(), x.cuda(), mean.cuda(), istd.cuda(), dw, db)
    assert rel(dw, wgt.grad.view(cc, 9)) < 1e-4 and rel(db, bias.grad) < 1e-4


def test_adam_and_overflow(K):
    g = torch.Generator().manual_seed(6)
    n = 100003
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1024
    p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.grad_overflow(gr.cuda(), flag)
    assert int(flag) == 0
    pm, mm, vm = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in (1, 2, 3):
        lr_t = 1e-3 * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        K.adam(p, gr.cuda(), m, v, lr_t, 0.9, 0.999, 1e-8, 1.0 / 1024, flag)
        gi = gr / 1024
        mm = 0.9 * mm + 0.1 * gi
        vm = 0.999 * vm + 0.001 * gi * gi
        pm = pm - lr_t * mm / (vm.sqrt() + 1e-8)
    assert rel(p, pm) < 1e-6
    bad = gr.clone()
    bad[777] = float("inf")
    K.grad_overflow(bad.cuda(), flag)
    assert int(flag) == 1
    before = p.clone()
    K.adam(p, gr.cuda(), m, v, 1e-3, 0.9, 0.999, 1e-8, 1.0, flag)
    assert torch.equal(p, before)  # update skipped on overflow
    # the update and the bf16 mirror of the new parameters in one launch (ma_adam_mirror_f32): the same parameter bits as ma_adam_f32, the
    # mirror = ma_cast_f32_bf16 of them; n % 4 != 0 is not covered (the caller casts); on overflow nothing is touched
    from mindaudio_amd import ops

    n4 = 100004
    p0, gr = torch.randn(n4, generator=g), torch.randn(n4, generator=g) * 1024
    flag.zero_()
    pa, ma_, va = p0.clone().cuda(), torch.zeros(n4, device="cuda"), torch.zeros(n4, device="cuda")
    pb, mb, vb = p0.clone().cuda(), torch.zeros(n4, device="cuda"), torch.zeros(n4, device="cuda")
    mir = torch.zeros(n4, dtype=torch.bfloat16, device="cuda")
    for step in (1, 2):
        lr_t = 1e-3 * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        assert K.adam(pa, gr.cuda(), ma_, va, lr_t, 0.9, 0.999, 1e-8, 1.0 / 1024, flag) is False
        assert K.adam(pb, gr.cuda(), mb, vb, lr_t, 0.9, 0.999, 1e-8, 1.0 / 1024, flag, mirror=mir) is True
        assert torch.equal(pa, pb) and torch.equal(ma_, mb) and torch.equal(va, vb)
        assert torch.equal(mir, ops.cast_bf16(pa.view(1, -1)).view(-1))
    assert K.adam(p, gr[:n].cuda(), m, v, 1e-3, 0.9, 0.999, 1e-8, 1.0, flag, mirror=torch.zeros(n, dtype=torch.bfloat16, device="cuda")) is False
    flag.fill_(1)
    keep_p, keep_m = pb.clone(), mir.clone()
    assert K.adam(pb, gr.cuda(), mb, vb, 1e-3, 0.9, 0.999, 1e-8, 1.0, flag, mirror=mir) is True
    assert torch.equal(pb, keep_p) and torch.equal(mir, keep_m)


@pytest.mark.parametrize("chunked", [False, True])
# (64, 255): 64 x 4 heads x 4 slabs = 1 024 workgroups per backward kernel (more than three resident rounds of 256 CUs)
# h = 8 / 12 / 16: d_model 512 / 768 / 1024 (round 6; the rows of qkv are [q (64 h) | k | v])
@pytest.mark.parametrize("b,t,h", [(2, 100, 4), (3, 255, 4), (1, 64, 4), (2, 37, 4), (2, 300, 4), (1, 129, 4), (64, 255, 4),
                                   (2, 100, 8), (2, 37, 12), (3, 255, 16), (20, 255, 8)])
def test_attention_backward(K, b, t, h, chunked):
    g = torch.Generator().manual_seed(7 + t)
    dk = 64
    dm = h * dk
    qkv = bf(torch.randn(b * t, 3 * dm, generator=g) * 0.8)
    pos = bf(torch.randn(t, dm, generator=g) * 0.8)
    u = (0.3 * torch.randn(h, dk, generator=g)).requires_grad_()
    v = (0.3 * torch.randn(h, dk, generator=g)).requires_grad_()
    lens = torch.randint(t // 2, t + 1, (b,), generator=g)
    lens[0] = t
    mask = (torch.arange(t)[None, :] < lens[:, None]).float()
    qf = qkv.float().requires_grad_()
    pf = pos.float().requires_grad_()
    q = qf[:, :dm].view(b, t, h, dk)
    k = qf[:, dm:2 * dm].view(b, t, h, dk).transpose(1, 2)
    vv = qf[:, 2 * dm:].view(b, t, h, dk).transpose(1, 2)
    p = pf.view(1, t, h, dk).transpose(1, 2)
    qu = bf((q + u).detach()).float() + ((q + u) - (q + u).detach())  # the kernels round q + bias to bf16 (straight-through)
    qv = bf((q + v).detach()).float() + ((q + v) - (q + v).detach())
    scores = (qu.transpose(1, 2) @ k.transpose(-1, -2) + qv.transpose(1, 2) @ p.transpose(-1, -2)) / math.sqrt(dk)
    if chunked:  # (B, T, T) per-(query, key) masks of the streaming configuration (utils/mask.py:201-271), padding folded in
        idx = torch.arange(t)
        chunk = ((idx[None, :] // 8) <= (idx[:, None] // 8)) & ((idx[None, :] // 8) >= (idx[:, None] // 8) - 2)
        mask = (chunk[None] & (mask[:, None, :] > 0)).float().contiguous()
        scores = scores + (mask[:, None] == 0).float() * -10000.0
    else:
        scores = scores + (mask[:, None, None, :] == 0).float() * -10000.0
    attn = torch.softmax(scores, -1)
    ctx_ref = (attn @ vv).transpose(1, 2).reshape(b * t, dm)
    dctx = bf(torch.randn(b * t, dm, generator=g))
    ctx_ref.backward(dctx.float())
    ctx, lse = K.attention_fwd(qkv.cuda(), pos.cuda(), u.detach().cuda(), v.detach().cuda(), mask.cuda(), b, t, heads=h)
    assert rel(ctx, ctx_ref.detach()) < 1e-2
    assert rel(lse, torch.logsumexp(scores.detach(), -1)) < 1e-3
    dpos = torch.zeros(t, dm, device="cuda")
    du, dv = torch.zeros(h, dk, device="cuda"), torch.zeros(h, dk, device="cuda")
    dqkv = K.attention_bwd(qkv.cuda(), pos.cuda(), u.detach().cuda(), v.detach().cuda(), mask.cuda(), ctx, dctx.cuda(),
                           lse, b, t, dpos, du, dv, heads=h)
    for name, lo in (("dq", 0), ("dk", dm), ("dv", 2 * dm)):
        assert rel(dqkv[:, lo:lo + dm], qf.grad[:, lo:lo + dm]) < 2e-2, name
    assert rel(dpos, pf.grad) < 2e-2
    assert rel(du, u.grad) < 2e-2 and rel(dv, v.grad) < 2e-2


def test_ctc_loss_grad(K):
    g = torch.Generator().manual_seed(11)
    b, t, v, lmax = 5, 61, 203, 12
    vp = (v + 63) // 64 * 64
    logits = torch.zeros(b * t, vp)
    logits[:, :v] = torch.randn(b * t, v, generator=g) * 2
    hlens = torch.tensor([61, 50, 33, 61, 4])
    ylens = torch.tensor([12, 7, 1, 0, 9])  # the last one is infeasible (9 labels in 4 frames): zero_infinity
    ys = torch.randint(1, v, (b, lmax), generator=g)
    ys[1, 3] = ys[1, 2]  # a repeated label
    lg = logits[:, :v].clone().view(b, t, v).requires_grad_()
    lp = torch.log_softmax(lg, -1).transpose(0, 1)
    per_ref = F.ctc_loss(lp, ys, hlens, ylens, blank=0, reduction="none", zero_infinity=True)
    (per_ref.sum() * 3.0).backward()
    loss, per, dlog = K.ctc_loss_grad(logits.cuda(), v, b, t, ys.cuda(), hlens.cuda(), ylens.cuda(), 3.0)
    want_per = per_ref.detach().clone()
    got_per = per.cpu()
    assert torch.isinf(got_per[4]) and want_per[4] == 0
    assert rel(got_per[:4], want_per[:4]) < 1e-5
    assert abs(float(loss) - float(want_per.sum()) / b) < 1e-4 * abs(float(want_per.sum()) / b)
    got = dlog.float().cpu().view(b, t, vp)
    assert float(got[..., v:].abs().max()) == 0.0
    assert rel(got[..., :v], lg.grad) < 5e-3
    assert float(got[4].abs().max()) == 0.0 and float(got[1, 50:].abs().max()) == 0.0


@pytest.mark.parametrize("lmax", [127, 128, 200, 223])
def test_ctc_loss_grad_long_targets(K, lmax):
    """Targets beyond 127 labels (conformer.yaml: token_max_length 200) run a 7-chunk instantiation of the recursion (round 6: they
    were refused); 127 is the last length of the 4-chunk form, 223 the last the library takes."""
    g = torch.Generator().manual_seed(lmax)
    b, t, v = 4, 2 * lmax + 40, 97
    vp = (v + 63) // 64 * 64
    logits = torch.zeros(b * t, vp)
    logits[:, :v] = torch.randn(b * t, v, generator=g) * 2
    hlens = torch.tensor([t, t - 17, lmax + 3, t])
    ylens = torch.tensor([lmax, lmax - 5, lmax, 3])  # (the third: lmax labels in lmax + 3 frames - feasible only without repeats)
    ys = torch.randint(1, v, (b, lmax), generator=g)
    ys[2] = (torch.arange(lmax) % (v - 1)) + 1       # no two neighbours equal
    ys[0, 10] = ys[0, 9]
    lg = logits[:, :v].clone().view(b, t, v).requires_grad_()
    lp = torch.log_softmax(lg, -1).transpose(0, 1)
    per_ref = F.ctc_loss(lp, ys, hlens, ylens, blank=0, reduction="none", zero_infinity=True)
    (per_ref.sum() * 2.0).backward()
    loss, per, dlog = K.ctc_loss_grad(logits.cuda(), v, b, t, ys.cuda(), hlens.cuda(), ylens.cuda(), 2.0)
    assert bool(torch.isfinite(per_ref).all()) and rel(per.cpu(), per_ref.detach()) < 1e-5
    got = dlog.float().cpu().view(b, t, vp)
    assert rel(got[..., :v], lg.grad) < 5e-3
    from mindaudio_amd import _lib

    with pytest.raises((NotImplementedError, _lib.MindaudioAmdError)):  # 224 labels: 449 states
        K.ctc_loss_grad(logits.cuda(), v, b, t, torch.ones(b, 224, dtype=torch.long).cuda(), hlens.cuda(), ylens.cuda(), 1.0)


def test_gemm_tn(K):
    g = torch.Generator().manual_seed(21)
    # (Kc, Mo, No, rows_store): tails in every dimension, small and large contractions
    for kc, mo, no, rs in ((10200, 256, 2048, None), (10200, 2048, 256, None), (255, 3072, 256, None), (1000, 768, 256, None),
                           (777, 4288, 256, 4233), (130, 64, 72, None), (64 * 9 + 1, 512, 256, None)):
        a, b = bf(torch.randn(kc, mo, generator=g)), bf(torch.randn(kc, no, generator=g))
        rs_ = mo if rs is None else rs
        out = torch.full((rs_, no), 0.5, device="cuda")
        cs = torch.zeros(mo, device="cuda")
        K.gemm_tn(a.cuda(), b.cuda(), out, colsum=cs, rows_store=rs, alpha=0.25)
        want = 0.5 + 0.25 * (a.float().t() @ b.float())[:rs_]
        assert rel(out, want) < 2e-5, (kc, mo, no)
        assert rel(cs[:rs_], a.float().sum(0)[:rs_]) < 2e-5, (kc, mo, no)
    # strided views (column slices of wider buffers)
    wide = bf(torch.randn(500, 1024, generator=g)).cuda()
    a, b = wide[:, 256:512], wide[:, 512:]
    out = torch.zeros(256, 512, device="cuda")
    K.gemm_tn(a, b, out, accumulate=False)
    assert rel(out, a.float().cpu().t() @ b.float().cpu()) < 2e-5


# lq > 32 (round 6): labels of more than 31 tokens - two or more query tiles, dk / dv summed over the tiles' launches
@pytest.mark.parametrize("lq,lk,mode", [(31, 31, 2), (31, 255, 1), (31, 749, 1), (9, 1088, 1), (32, 321, 0),
                                        (45, 45, 2), (61, 255, 1), (33, 749, 1), (201, 201, 2), (64, 300, 0)])
def test_decoder_attention_long_sources(K, lq, lk, mode):
    """ma_mha_small_fwd/bwd (the TransformerDecoder's self- and source attention, layers/attention.py:85-157 with the 1/d_k
    scaling of :150-152) over short AND long key ranges: up to 320 keys the V / K rows are staged in LDS, beyond that (the
    1400 ... 3000-frame buckets of conformer.yaml: T' up to 749) the score rows take the LDS and V / K come from L2.  Forward and
    every gradient against float32 autograd on the same bf16-rounded inputs."""
    g = torch.Generator().manual_seed(lq * 1000 + lk)
    b, h, dk = 3, 4, 64
    scale = 1.0 / dk
    q = bf(torch.randn(b * lq, h * dk, generator=g))
    k = bf(torch.randn(b * lk, h * dk, generator=g) * 4)
    v = bf(torch.randn(b * lk, h * dk, generator=g))
    dctx = bf(torch.randn(b * lq, h * dk, generator=g))
    if mode == 1:
        mask = torch.ones(b, lk)
        mask[1, lk - lk // 3:] = 0
        mask[2, lk // 2:] = 0
        add = (mask == 0).float()[:, None, None, :] * -10000.0
    elif mode == 2:
        mask = torch.tril(torch.ones(lq, lk))[None].repeat(b, 1, 1).contiguous()
        mask[2, :, lk - 5:] = 0
        add = (mask == 0).float()[:, None] * -10000.0
    else:
        mask, add = None, 0.0
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    q4 = qf.view(b, lq, h, dk).transpose(1, 2)
    k4 = kf.view(b, lk, h, dk).transpose(1, 2)
    v4 = vf.view(b, lk, h, dk).transpose(1, 2)
    probs_ref = torch.softmax(q4 @ k4.transpose(-1, -2) * scale + add, dim=-1)
    ctx_ref = (probs_ref @ v4).transpose(1, 2).reshape(b * lq, h * dk)
    ctx_ref.backward(dctx.float())
    ctx, probs = K.mha_small_fwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda() if mask is not None else None, mode, b, lq, lk, scale,
                                 h, dk)
    assert rel(probs, probs_ref.detach()) < 2e-5
    assert rel(ctx, ctx_ref.detach()) < 4e-3          # bf16 output rounding
    dq, dk_, dv = (torch.empty_like(t.cuda()) for t in (q, k, v))
    K.mha_small_bwd(q.cuda(), k.cuda(), v.cuda(), probs, ctx, dctx.cuda(), b, lq, lk, scale, dq, dk_, dv, h, dk)
    assert rel(dq, qf.grad) < 1e-2 and rel(dk_, kf.grad) < 1e-2 and rel(dv, vf.grad) < 6e-3
    # ... and the float32 form (the validation mode's kernels): same tiling, exact accumulation over the query tiles
    from mindaudio_amd.train import kernels_x32 as X

    ctx32, probs32 = X.mha_small_fwd(q.float().cuda(), k.float().cuda(), v.float().cuda(), mask.cuda() if mask is not None else None,
                                     mode, b, lq, lk, scale, h, dk)
    assert rel(probs32, probs_ref.detach()) < 2e-5 and rel(ctx32, ctx_ref.detach()) < 2e-5
    dq32, dk32, dv32 = (torch.empty_like(t.float().cuda()) for t in (q, k, v))
    X.mha_small_bwd(q.float().cuda(), k.float().cuda(), v.float().cuda(), probs32, ctx32, dctx.float().cuda(), b, lq, lk, scale,
                    dq32, dk32, dv32, h, dk)
    assert rel(dq32, qf.grad) < 2e-5 and rel(dk32, kf.grad) < 2e-5 and rel(dv32, vf.grad) < 2e-5


def test_decoder_attention_rejects_more_keys_than_the_lds_holds(K):
    b, h, dk, lq, lk = 1, 4, 64, 4, 1089
    z = lambda n: torch.zeros(n, h * dk, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    with pytest.raises(NotImplementedError):
        K.mha_small_fwd(z(lq), z(lk), z(lk), None, 0, b, lq, lk, 1.0 / dk, h, dk)


@pytest.mark.parametrize("m,k,p", [(1240, 2048, 0.1), (1240, 2048, 0.0), (37, 512, 0.3), (5000, 4288 + 64, 0.1)])
def test_split_k_join_equals_its_four_launches_bit_for_bit(K, m, k, p):
    """ma_gemm_bf16_splitk_join_f32 (the TransformerDecoder's w_2 + dropout + residual + the next LayerNorm, models/conformer.py:430-470,
    501-530) against ma_gemm_bf16_splitk_f32 + bias + a bf16 rounding + ma_dropout_add_f32 + ma_layernorm_f32: the same splits summed
    in the same order, the same mask - the joined rows bit-identical, their LayerNorm to one bf16 ulp; and against float64."""
    from mindaudio_amd import ops

    g = torch.Generator().manual_seed(m + k)
    a = bf(torch.randn(m, k, generator=g)).cuda()
    w = bf(torch.randn(256, k, generator=g) / math.sqrt(k)).cuda()
    bias, x = torch.randn(256, generator=g).cuda(), torch.randn(m, 256, generator=g).cuda()
    g1, b1 = (1 + 0.1 * torch.randn(256, generator=g)).cuda(), (0.1 * torch.randn(256, generator=g)).cuda()
    seed, salt = 4242, 17
    out, ln = K.dense_join_splitk(a, w, bias, x, 0.5, p, seed, salt, ln1=(g1, b1), eps=1e-12)
    y = K.gemm_splitk(a, w, torch.empty(m, 256, device="cuda"), accumulate=False)
    z = (y + bias).to(torch.bfloat16)
    want = K.dropout_add(x, z, 0.5, p, seed, salt)
    want_ln = ops.layernorm(want, g1, b1, eps=1e-12)
    assert torch.equal(out, want)
    # (the LayerNorm of the bit-identical rows: the compiler contracts the two kernels' multiply-adds differently - one bf16 ulp)
    assert float(((ln.float() - want_ln.float()).abs() - 2.0 ** -7 * want_ln.float().abs()).max()) <= 1e-6  # (1e-6: float32 noise at a zero crossing)
    assert float((ln != want_ln).float().mean()) < 0.02
    out2, none = K.dense_join_splitk(a, w, None, None, 1.0, p, seed, salt)  # no bias, no residual, no LayerNorm
    assert none is None and torch.equal(out2, K.dropout_add(None, y.to(torch.bfloat16), 1.0, p, seed, salt))
    if p == 0.0:
        ref = x.double().cpu() + 0.5 * (a.double().cpu() @ w.double().cpu().t() + bias.double().cpu())
        # (one bf16 rounding of z = a W^T + b, |z| = 2 |ref - x| at alpha = 0.5: half an ulp of the largest z)
        assert float((out.double().cpu() - ref).abs().max()) < 2 ** -8 * float((ref - x.double().cpu()).abs().max()) + 1e-4
        mu, var = ref.mean(1, keepdim=True), ref.var(1, unbiased=False, keepdim=True)
        ref_ln = (ref - mu) / torch.sqrt(var + 1e-12) * g1.double().cpu() + b1.double().cpu()
        assert float((ln.double().cpu() - ref_ln).abs().max()) < 0.05


def test_split_k_join_rejects_what_it_does_not_do(K):
    import ctypes

    from mindaudio_amd import _host, _lib

    lib = _lib.load()
    a, w = torch.zeros(64, 512, dtype=torch.bfloat16, device="cuda"), torch.zeros(256, 512, dtype=torch.bfloat16, device="cuda")
    out, ws = torch.zeros(64, 256, device="cuda"), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    st = _host.current_stream_ptr()
    e = K._train_epi(3)
    call = lambda n, epi, nbytes: lib.ma_gemm_bf16_splitk_join_f32(a.data_ptr(), 512, w.data_ptr(), 512, out.data_ptr(), 256, 64, n,  # noqa: E731
                                                                   512, ctypes.byref(epi), ws.data_ptr(), nbytes, st)
    assert call(256, e, ws.numel()) == 0
    assert call(512, e, ws.numel()) == _lib.MA_ERR_UNSUPPORTED  # a join is 256 wide
    assert call(256, K._train_epi(4), ws.numel()) == _lib.MA_ERR_UNSUPPORTED  # only the join mode
    assert call(256, e, 1024) == _lib.MA_ERR_WORKSPACE
    torch.cuda.synchronize()


def test_fused_dense_layers_equal_their_unfused_launches(K):
    """ma_gemm_k256_train_bf16 / ma_gemm_rows_train_bf16 / ma_layernorm_bwd_next_f32 against the launches they replace, same dropout
    sites: u, h, du and the emitted dy are BIT-identical (same products, same rounding points, same masks); the join's float32 output
    and LayerNorms agree to float32 / one bf16 ulp (the fused join does not round the residual sum's input twice)."""
    from mindaudio_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    m, d, hid, p, seed = 1000, 256, 2048, 0.1, 12345
    st = torch.cuda.current_stream().cuda_stream

    def pack(w, kind):
        n, k = w.shape
        pieces = int(lib.ma_pack_item_pieces(kind, n, k))
        out = torch.empty(pieces * 16, dtype=torch.uint8, device="cuda")
        items = (_lib.PackItem * 1)(_lib.PackItem(w.data_ptr(), out.data_ptr(), w.stride(0), n, k, kind, 0))
        d_items = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).cuda()
        d_map = torch.zeros((pieces + 255) // 256, dtype=torch.int32, device="cuda")
        _lib.check(lib.ma_pack_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), d_map.numel(), st), "pack")
        return out

    a = bf(torch.randn(m, d, generator=g)).cuda()
    w1 = bf(torch.randn(hid, d, generator=g) / 16).cuda()
    w2 = bf(torch.randn(d, hid, generator=g) / 45).cuda()
    b1, b2 = torch.randn(hid, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    x = torch.randn(m, d, generator=g).cuda()
    rs = (torch.rand(m, generator=g) > 0.2).float().cuda()
    g1, be1 = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    g2, be2 = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    # ---- w_1 forward: u, h
    u_ref = ops.gemm(a, w1, bias=b1)
    h_ref = K.act_dropout_fwd(u_ref, p, seed, 3)
    u, h = K.dense_act_drop(a, pack(w1, 0), hid, b1, p, seed, 3)
    assert torch.equal(u, u_ref) and torch.equal(h, h_ref)
    # ... and with ReLU (ma_train_epilogue_t.act = 2, round 6: the TransformerDecoder's feed-forward), forward and backward, M = 1 240
    from mindaudio_amd import _lib as L_
    ar = bf(torch.randn(1240, d, generator=g)).cuda()
    ur_ref = ops.gemm(ar, w1, bias=b1)
    hr_ref = K.act_dropout_fwd(ur_ref, p, seed, 5, act=L_.ACT_RELU)
    ur, hr = K.dense_act_drop(ar, pack(w1, 0), hid, b1, p, seed, 5, act=L_.ACT_RELU)
    assert torch.equal(ur, ur_ref) and torch.equal(hr, hr_ref)
    assert float((hr == 0).float().mean()) > 0.5 and not torch.equal(hr, K.dense_act_drop(ar, pack(w1, 0), hid, b1, p, seed, 5)[1])
    dyr = bf(torch.randn(1240, d, generator=g)).cuda()
    w2t = w2.t().contiguous()  # (hid, 256): dh = dy . W2
    dh_ref = ops.gemm(dyr, w2t)
    du_ref = K.act_dropout_bwd(ur_ref, dh_ref, p, seed, 5, act=L_.ACT_RELU)
    du = K.dense_act_drop_bwd(dyr, pack(w2t, 0), hid, ur_ref, p, seed, 5, act=L_.ACT_RELU)
    assert torch.equal(du, du_ref)
    # ---- w_2 forward + dropout + residual (+ LayerNorm chain)
    y_ref = ops.gemm(h, w2, bias=b2, row_scale=rs)
    x_ref = K.dropout_add(x, y_ref, 0.5, p, seed, 4)
    ln_ref = ops.layernorm(x_ref, g1, be1, row_scale=rs)
    for kind_w, kk, src in ((pack(w2, 1), hid, h),):
        xo, lo, _ = K.dense_join(src, kind_w, kk, b2, x, 0.5, p, seed, 4, row_scale=rs, ln1=(g1, be1), ln_row_scale=rs)
        assert torch.equal(xo, x_ref)
        assert float((lo.float() - ln_ref.float()).abs().max()) <= 2 ** -6  # one bf16 ulp at |v| < 4
        assert rel(lo, ln_ref.float().cpu()) < 2e-3
        xo2, lo2, mid2 = K.dense_join(src, kind_w, kk, b2, x, 0.5, p, seed, 4, row_scale=rs, ln1=(g1, be1), ln2=(g2, be2))
        mid_ref = ops.layernorm(x_ref, g1, be1, out_dtype=torch.float32)
        ln2_ref = ops.layernorm(mid_ref, g2, be2)
        assert torch.equal(xo2, x_ref) and rel(mid2, mid_ref.cpu()) < 1e-5 and rel(lo2, ln2_ref.float().cpu()) < 2e-3
    # the K = 256 join (linear_out / pointwise_conv2)
    wo = bf(torch.randn(d, d, generator=g) / 16).cuda()
    yo_ref = ops.gemm(a, wo, bias=b2)
    xo_ref = K.dropout_add(x, yo_ref, 1.0, p, seed, 5)
    xo, lo, _ = K.dense_join(a, pack(wo, 0), d, b2, x, 1.0, p, seed, 5, ln1=(g1, be1))
    assert torch.equal(xo, xo_ref) and rel(lo, ops.layernorm(xo_ref, g1, be1).float().cpu()) < 2e-3
    # ---- w_1 backward: dh -> du on the packed transposed w_2
    dy = bf(torch.randn(m, d, generator=g)).cuda()
    w2t = w2.t().contiguous()                     # (hid, d): rows = hidden units
    dh_ref = ops.gemm(dy, w2t)
    du_ref = K.act_dropout_bwd(u_ref, dh_ref, p, seed, 3)
    du = K.dense_act_drop_bwd(dy, pack(w2t, 0), hid, u_ref, p, seed, 3)
    assert torch.equal(du, du_ref)
    # ---- plain products on packed weights: K = 2048 / 768 / 512 -> 256 and 256 -> 768
    for kk in (hid, 768, 512):
        src = bf(torch.randn(m, kk, generator=g)).cuda()
        w = bf(torch.randn(d, kk, generator=g) / 30).cuda()
        assert torch.equal(K.dense_plain(src, pack(w, 1), d, kk), ops.gemm(src, w))
    wq = bf(torch.randn(768, d, generator=g) / 16).cuda()
    bq = torch.randn(768, generator=g).cuda()
    assert torch.equal(K.dense_plain(a, pack(wq, 0), 768, d, bias=bq), ops.gemm(a, wq, bias=bq))
    # ---- LayerNorm backward that also emits the next branch's dropout backward
    dyl = bf(torch.randn(m, d, generator=g)).cuda()
    ga = (1 + 0.1 * torch.randn(d, generator=g)).cuda()
    gacc = torch.randn(m, d, generator=g).cuda()
    g_ref, dg_ref, db_ref = gacc.clone(), torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    K.layernorm_bwd(x, ga, dyl, g_ref, dg_ref, db_ref, row_scale=rs)
    dn_ref = K.dropout_bwd(g_ref, 0.5, p, seed, 6, row_scale=rs)
    g_new, dg, db = gacc.clone(), torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    _, dn = K.layernorm_bwd_next(x, ga, dyl, g_new, dg, db, (0.5, p, seed, 6, rs), row_scale=rs)
    assert torch.equal(g_new, g_ref) and torch.equal(dn, dn_ref) and torch.equal(dg, dg_ref) and torch.equal(db, db_ref)


# (40000, 2048): 834 workgroups of 48 rows = more than three resident rounds, against float64 like the others
@pytest.mark.parametrize("m,hid,chain", [(1000, 2048, True), (10200, 2048, False), (49, 256, False), (48, 512, True), (1, 256, False),
                                         (40000, 2048, True)])
def test_feed_forward_module_in_one_launch(K, m, hid, chain):
    """ma_ffn_train_bf16 against the two launches it replaces (ma_gemm_k256_train_bf16 mode 1 + ma_gemm_rows_train_bf16 mode 3, same
    dropout sites) and against float64: the dropout masks are the SAME element for element; u differs by at most one bf16 ulp (the
    bias enters the float32 accumulation first instead of last), h by the rounding of Swish's argument, the join by the order of the
    hidden units' sum."""
    from mindaudio_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator().manual_seed(5 + m)
    d, p, seed = 256, 0.1, 4242
    st = torch.cuda.current_stream().cuda_stream
    a = bf(torch.randn(m, d, generator=g)).cuda()
    w1 = bf(torch.randn(hid, d, generator=g) / 16).cuda()
    w2 = bf(torch.randn(d, hid, generator=g) / 45).cuda()
    b1, b2 = torch.randn(hid, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    x = torch.randn(m, d, generator=g).cuda()
    g1, be1 = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    g2, be2 = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()

    def pack(w, kind, out=None):
        n, k = w.shape
        pieces = int(lib.ma_pack_item_pieces(kind, n, k))
        assert pieces > 0
        if out is None:
            out = torch.empty(pieces * 16 * (2 if kind in (2, 3) else 1), dtype=torch.uint8, device="cuda")
        items = (_lib.PackItem * 1)(_lib.PackItem(w.data_ptr(), out.data_ptr(), w.stride(0), n, k, kind, 0))
        d_items = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).cuda()
        d_map = torch.zeros((pieces + 255) // 256, dtype=torch.int32, device="cuda")
        _lib.check(lib.ma_pack_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), d_map.numel(), st), "pack")
        return out

    # the two halves written by the batched packer == the evaluation path's packer
    pk = pack(w2, 3, pack(w1, 2))
    assert torch.equal(pk, ops.ffn_pack_weights(w1, w2).view(torch.uint8).reshape(-1))
    ln2 = (g2, be2) if chain else None
    u, h, xo, lo, mid = K.ffn_train(a, pk, hid, b1, p, seed, 3, b2, x, 0.5, p, 4, ln1=(g1, be1), ln2=ln2)
    u_ref, h_ref = K.dense_act_drop(a, pack(w1, 0), hid, b1, p, seed, 3)
    xo_ref, lo_ref, mid_ref = K.dense_join(h_ref, pack(w2, 0 if hid == 256 else 1), hid, b2, x, 0.5, p, seed, 4, ln1=(g1, be1), ln2=ln2)
    # u: one bf16 ulp
    du = (u.float() - u_ref.float()).abs()
    assert float((du / u_ref.float().abs().clamp_min(2.0 ** -6)).max()) <= 2.0 ** -7
    # the hidden dropout mask: identical wherever swish(u) does not round to zero by itself
    big = u_ref.float().abs() > 1e-3
    assert torch.equal((h == 0) & big, (h_ref == 0) & big)
    frac = float(((h == 0) & big).float().mean())
    assert abs(frac - p) < (0.02 if m * hid > 50000 else 0.06), frac
    # h against float64 on the float32 pre-activation
    u64 = a.double() @ w1.double().t() + b1.double()
    h64 = u64 * torch.sigmoid(u64) / (1 - p) * (h_ref != 0).double()
    sel = big & (h_ref != 0)
    assert float(((h.double() - h64).abs() / h64.abs().clamp_min(1e-2))[sel].max()) < 2.0 ** -7  # < 1 bf16 ulp (+ fast sigmoid)
    assert rel(h, h_ref.float().cpu()) < 5e-3  # (Swish of the bf16-rounded u in the two-launch form: 2^-9 relative, rms)
    # the join: float64 on THIS launch's h and the join's own mask (recovered from the two-launch result: z = 0 <=> dropped)
    z64 = h.double() @ w2.double().t() + b2.double()
    keep = ((xo_ref - x) != 0).double()
    xo64 = x.double() + 0.5 * z64 * keep / (1 - p)
    err = (xo.double() - xo64).abs()
    assert float(err.max()) < 2.0 ** -8 * float(z64.abs().max()) + 1e-5, float(err.max())
    assert rel(xo, xo_ref.cpu()) < 2e-3
    if chain:
        assert rel(mid, mid_ref.cpu()) < 2e-3 and rel(lo, lo_ref.float().cpu()) < 4e-3
        mid64 = torch.nn.functional.layer_norm(xo.double(), (d,), g1.double(), be1.double(), 1e-5)
        lo64 = torch.nn.functional.layer_norm(mid64, (d,), g2.double(), be2.double(), 1e-5)
        assert rel(mid, mid64.cpu()) < 1e-5 and rel(lo, lo64.cpu()) < 3e-3
    else:
        assert mid is None
        lo64 = torch.nn.functional.layer_norm(xo.double(), (d,), g1.double(), be1.double(), 1e-5)
        assert rel(lo, lo64.cpu()) < 3e-3 and rel(lo, lo_ref.float().cpu()) < 4e-3
    # bad arguments
    with pytest.raises(Exception):
        K.ffn_train(a, pk, hid + 64, b1, p, seed, 3, b2, x, 0.5, p, 4)


@pytest.mark.parametrize("m,hid", [(1000, 2048), (10200, 2048), (49, 256), (1, 512), (40000, 2048)])
def test_feed_forward_module_backward_in_one_launch(K, m, hid):
    """ma_ffn_train_bwd_bf16 (dh -> du -> da -> LayerNorm backward, one launch, on the gk = swish' * keep / (1 - p) tape of the one-launch
    forward) against float64 and against the two launches it replaces (ma_gemm_k256_train_bf16 mode 2 on the bf16 u of the two-launch
    forward, ma_gemm_rows_train_bf16 mode 5): du within bf16 round-off of both (gk carries one more bf16 rounding, u's rounding is
    gone), g / dgamma / dbeta / dy_next computed from THIS launch's du agree with the two-launch LayerNorm backward on the same du to
    float32 round-off."""
    from mindaudio_amd import _lib, ops

    lib = _lib.load()
    gen = torch.Generator().manual_seed(31 + m)
    d, p, seed = 256, 0.1, 99
    st = torch.cuda.current_stream().cuda_stream

    def pack(w, kind, out=None):
        n, k = w.shape
        pieces = int(lib.ma_pack_item_pieces(kind, n, k))
        assert pieces > 0
        if out is None:
            out = torch.empty(pieces * 16 * (2 if kind in (2, 3) else 1), dtype=torch.uint8, device="cuda")
        items = (_lib.PackItem * 1)(_lib.PackItem(w.data_ptr(), out.data_ptr(), w.stride(0), n, k, kind, 0))
        d_items = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).cuda()
        d_map = torch.zeros((pieces + 255) // 256, dtype=torch.int32, device="cuda")
        _lib.check(lib.ma_pack_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), d_map.numel(), st), "pack")
        return out

    a = bf(torch.randn(m, d, generator=gen)).cuda()
    w1 = bf(torch.randn(hid, d, generator=gen) / 16).cuda()
    w2 = bf(torch.randn(d, hid, generator=gen) / 45).cuda()
    b1, b2 = torch.randn(hid, generator=gen).cuda(), torch.randn(d, generator=gen).cuda()
    x = torch.randn(m, d, generator=gen).cuda() * 2 + 0.3       # the module's residual input = the LayerNorm's input
    gamma = (1 + 0.1 * torch.randn(d, generator=gen)).cuda()
    dy = bf(torch.randn(m, d, generator=gen)).cuda()
    g0 = torch.randn(m, d, generator=gen).cuda()
    w1t, w2t = w1.t().contiguous(), w2.t().contiguous()         # (256, hid), (hid, 256)
    # forward tapes: gk from the one-launch forward, u from the two-launch forward
    gk, h, _, _, _ = K.ffn_train(a, pack(w2, 3, pack(w1, 2)), hid, b1, p, seed, 3, b2, x, 0.5, p, 4, tape_derivative=True)
    u_ref, h_ref = K.dense_act_drop(a, pack(w1, 0), hid, b1, p, seed, 3)
    u64 = a.double() @ w1.double().t() + b1.double()
    sg = torch.sigmoid(u64)
    gk64 = sg * (1 + u64 * (1 - sg)) / (1 - p) * (h_ref != 0).double()
    sel = u_ref.float().abs() > 1e-3
    assert torch.equal((gk == 0) & sel, (h_ref == 0) & sel)
    assert float(((gk.double() - gk64).abs() / gk64.abs().clamp_min(1e-2))[sel].max()) < 2.0 ** -7
    pt = pack(w1t, 3, pack(w2t, 2))
    assert torch.equal(pt, ops.ffn_pack_weights(w2t, w1t).view(torch.uint8).reshape(-1))
    for nxt in ((0.5, p, seed, 9, None), None):
        g_new = g0.clone()
        parts = torch.full((K.ffn_train_parts(m) * 512,), float("nan"), device="cuda")
        du, dn = K.ffn_train_bwd(dy, pt, hid, gk, x, gamma, g_new, parts, nxt=nxt)
        torch.cuda.synchronize()
        # du: float64 on the stored gk, and the two-launch du
        dh = bf(dy.double() @ w2.double()).double()
        du64 = dh * gk.double()
        # (one bf16 ulp of dh - the kernel rounds its float32 sum, the reference the exact one - plus du's own rounding)
        assert float(((du.double() - du64).abs() / du64.abs().clamp_min(1e-2)).max()) < 2.0 ** -6
        du_ref = K.dense_act_drop_bwd(dy, pack(w2t, 0), hid, u_ref, p, seed, 3)
        assert rel(du, du_ref.float().cpu()) < 6e-3
        # the LayerNorm backward on THIS du: the two-launch form
        g_ref, dg_ref, db_ref = g0.clone(), torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
        da = K.dense_plain(du, pack(w1t, 0 if hid == 256 else 1), d, hid)
        if nxt is None:
            K.layernorm_bwd(x, gamma, da, g_ref, dg_ref, db_ref)
            assert dn is None
        else:
            _, dn_ref = K.layernorm_bwd_next(x, gamma, da, g_ref, dg_ref, db_ref, nxt)
            a_, b_ = dn.float(), dn_ref.float()
            assert torch.equal(a_ == 0, b_ == 0)
            diff = (a_ - b_).abs()
            # (da sums the hidden units in another order: where its bf16 rounding flips, dy_next moves by a few bf16 ulps; the bound is
            # on the MAXIMUM over m * 256 elements - the 40 000-row case draws four times the samples of the 10 200-row one)
            assert float((diff / b_.abs().clamp(min=1e-2)).max()) <= (3.0 / 16 if m > 20000 else 1.0 / 8)
            assert rel(a_, b_.cpu()) < 4e-3
        # (da is not rounded to bf16 on its way into the LayerNorm backward here: bf16 round-off of da against the two launches)
        scale = float(g_ref.abs().max())
        assert float((g_new - g_ref).abs().max()) <= 2e-2 * scale
        assert rel(g_new - g0, (g_ref - g0).cpu()) < 4e-3
        pv = parts.view(-1, 512).double().sum(0)
        assert bool(torch.isfinite(pv).all())
        assert rel(pv[:256].float(), dg_ref.cpu()) < 4e-3 and rel(pv[256:].float(), db_ref.cpu()) < 4e-3
    # ---- chain: a second LayerNorm backward on the finished rows (norm_final of the block below), g replaced, dy_next from it
    x2 = torch.randn(m, d, generator=gen).cuda() * 1.5 - 0.2
    gamma2 = (1 + 0.1 * torch.randn(d, generator=gen)).cuda()
    nxt2 = (0.5, p, seed, 11, None)
    g_new = g0.clone()
    parts = torch.full((K.ffn_train_parts(m) * 512,), float("nan"), device="cuda")
    parts2 = torch.full((K.ffn_train_parts(m) * 512,), float("nan"), device="cuda")
    du, dn = K.ffn_train_bwd(dy, pt, hid, gk, x, gamma, g_new, parts, chain=(x2, gamma2, parts2, nxt2))
    # reference: the un-chained launch, then the stand-alone LayerNorm backward that replaces g
    g_ref = g0.clone()
    parts_r = torch.zeros_like(parts)
    du_r, none = K.ffn_train_bwd(dy, pt, hid, gk, x, gamma, g_ref, parts_r)
    assert none is None and torch.equal(du, du_r)
    dg2, db2 = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    _, dn_ref = K.layernorm_bwd_next(x2, gamma2, g_ref, g_ref, dg2, db2, nxt2, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(parts, parts_r)  # the first LayerNorm's partials do not change
    scale = float(g_ref.abs().max())
    assert float((g_new - g_ref).abs().max()) <= 2e-5 * scale + 1e-6
    pv2 = parts2.view(-1, 512).double().sum(0)
    assert float((pv2[:256] - dg2.double()).abs().max()) <= 5e-5 * float(dg2.abs().max()) + 1e-5
    assert float((pv2[256:] - db2.double()).abs().max()) <= 5e-5 * float(db2.abs().max()) + 1e-5
    a_, b_ = dn.float(), dn_ref.float()
    assert torch.equal(a_ == 0, b_ == 0)
    diff = (a_ - b_).abs()
    assert float((diff / b_.abs().clamp(min=1e-3)).max()) <= 1.0 / 64 and float((diff > 0).float().mean()) < 5e-3


@pytest.mark.parametrize("b,h,w,c", [(2, 21, 19, 128), (3, 24, 39, 256), (1, 3, 3, 128), (2, 8, 6, 128), (9, 187, 39, 256),
                                     (8, 206, 40, 256)])
def test_conv2_input_gradient_as_one_implicit_gemm(K, b, h, w, c):
    """ma_conv2d_3x3s2_dinput_bf16 (parity-class implicit GEMM) against torch's conv_transpose2d on the same bf16 operands in float32
    (tolerance: one bf16 rounding of the result), and against the two-launch form it replaces (dy . W, then col2im + ReLU').  Even and
    odd H / W (rows and columns that no window covers get a zero gradient), the 3 x 3 image (one window), with and without ReLU'.
    The last two shapes (C = 256, >= 65 536 input positions) run the 256 x 256-tile kernel of round 4 (conv2_dinput8_kernel)."""
    from mindaudio_amd import ops

    g = torch.Generator().manual_seed(1000 * h + w)
    act = bf(torch.relu(torch.randn(b, h, w, c, generator=g)))
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    dy = bf(torch.randn(b * ho * wo, c, generator=g))
    wgt = bf(torch.randn(c, 3, 3, c, generator=g) / 30)                      # (co, kh, kw, c): the layout the step keeps
    wt = wgt.view(c, 9 * c).t().contiguous()                                  # ((kh, kw, c), co)
    full = F.conv_transpose2d(dy.float().view(b, ho, wo, c).permute(0, 3, 1, 2), wgt.float().permute(0, 3, 1, 2), stride=2)
    want = torch.zeros(b, c, h, w)
    want[:, :, :full.shape[2], :full.shape[3]] = full[:, :, :h, :w]
    want = want.permute(0, 2, 3, 1)
    got_nomask = K.conv2_dinput(dy.cuda(), wt.cuda(), act.cuda())              # with ReLU'
    assert rel(got_nomask, bf(want * (act.float() > 0)).float()) < 3e-3
    assert torch.equal(got_nomask.cpu() == 0, ((want * (act.float() > 0)) == 0) | (got_nomask.cpu() == 0))
    assert float(got_nomask.float().cpu()[act.float() <= 0].abs().max()) == 0.0
    # the two-launch form: same value up to its extra bf16 rounding of every tap
    dcol = ops.gemm(dy.cuda(), wt.cuda())
    two = K.col2im_relu(dcol, act.cuda())
    assert rel(got_nomask, two.float().cpu()) < 8e-3


def test_grouped_weight_gradient_products_equal_the_separate_launches(K):
    """ma_gemm_tn_partial_group_bf16 (a block's eight dW = dY^T X products as one grid) writes the same split-K partials and partial
    bias sums as eight ma_gemm_tn_partial_bf16 launches, bit for bit; more than eight items go out as two grids."""
    from mindaudio_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(77)
    m = 1531
    shapes = [(256, 2048), (2048, 256), (768, 256), (256, 256), (512, 256), (256, 256), (2048, 256), (256, 2048), (256, 512), (64, 128)]
    ops_ = []
    for mo, no in shapes:
        a = bf(torch.randn(m, mo, generator=g)).cuda()
        b = bf(torch.randn(m, no, generator=g)).cuda()
        nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, m))
        ops_.append((a, b, nbytes))
    sep = []
    for a, b, nbytes in ops_:
        part = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda")
        K.gemm_tn_partial(a, b, part, with_colsum=True)
        sep.append(part)
    grp = [torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda") for _, _, nbytes in ops_]
    K.gemm_tn_partial_group([(a, b, part) for (a, b, _), part in zip(ops_, grp)], with_colsum=True)
    for x, y in zip(sep, grp):
        assert torch.equal(x, y)



@pytest.mark.parametrize("kc", [10200, 64, 37, 1531])
def test_direct_weight_gradient_products_no_split_k(K, kc):
    """ma_gemm_tn_direct_group_bf16 (round 4): out = A^T B and the column sums of A for a list of products in ONE grid of 256 x 256
    tiles, every tile with the full contraction (no split-K partials, no reduction pass), stored straight into strided outputs.
    Against float64 products of the same bf16 operands: 2e-5 of the output scale (float32 accumulation over up to 10 200 rows)."""
    g = torch.Generator().manual_seed(78 + kc)
    shapes = [(256, 2048), (2048, 256), (768, 256), (256, 256), (512, 256), (256, 512)]
    quads, want = [], []
    for n, (mo, no) in enumerate(shapes):
        lda = mo + (64 if n % 2 else 0)  # strided operands: slices of wider activations
        a_full = bf(torch.randn(kc, lda, generator=g)).cuda()
        b_full = bf(torch.randn(kc, no + 8, generator=g)).cuda()
        a, b = a_full[:, :mo], b_full[:, :no]
        out_full = torch.full((mo, no + 4), 7.0, device="cuda")
        out = out_full[:, :no]
        cs = torch.full((mo,), 7.0, device="cuda") if n != 3 else None
        quads.append((a, b, out, cs))
        want.append((a.double().t() @ b.double(), a.double().sum(0), out_full))
        assert K.gemm_tn_direct_ok(a, b, out)
    K.gemm_tn_direct_group(quads)
    torch.cuda.synchronize()
    for (a, b, out, cs), (w, wcs, out_full) in zip(quads, want):
        scale = float(w.abs().max())
        assert float((out.double() - w).abs().max()) <= 2e-5 * scale
        assert bool((out_full[:, out.shape[1]:] == 7.0).all())  # nothing written past the row
        if cs is not None:
            assert float((cs.double() - wcs).abs().max()) <= 2e-5 * max(float(wcs.abs().max()), 1.0) + 1e-4
    # 50 products: two grids; and a shape the kernel refuses
    many = [quads[i % len(quads)] for i in range(50)]
    K.gemm_tn_direct_group(many)
    torch.cuda.synchronize()
    assert float((many[-1][2].double() - want[49 % len(quads)][0]).abs().max()) <= 2e-5 * float(want[49 % len(quads)][0].abs().max())
    odd = bf(torch.randn(kc, 192)).cuda()
    assert not K.gemm_tn_direct_ok(odd, quads[0][1], torch.empty(192, 2048, device="cuda"))


@pytest.mark.parametrize("b2,h2,w2", [(2, 23, 19), (9, 67, 39)])
def test_conv2_weight_gradient_on_256_tiles(K, b2, h2, w2):
    """C = Cout = 256 (the subsampling layer's shape): ma_conv2d_3x3s2_dw_bf16 routes to the 256 x 256-tile kernel
    (gemm_tn8_conv_kernel: implicit im2col operand, contraction split over the grid's second axis, partials added in split order);
    against autograd of F.conv2d on the same bf16 operands.  The second shape has enough rows for several splits and a K-tile tail."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(5 + b2)
    c2 = co2 = 256
    act_b = bf(torch.randn(b2, h2, w2, c2, generator=g))
    ho2, wo2 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    dy_b = bf(torch.randn(b2 * ho2 * wo2, co2, generator=g))
    wgt2 = torch.zeros(co2, c2, 3, 3, requires_grad=True)
    bias2 = torch.zeros(co2, requires_grad=True)
    o2 = F.conv2d(act_b.float().permute(0, 3, 1, 2), wgt2, bias2, stride=2)
    o2.backward(dy_b.float().view(b2, ho2, wo2, co2).permute(0, 3, 1, 2))
    from mindaudio_amd import _lib

    rows = b2 * ho2 * wo2
    assert int(_lib.load().ma_conv2d_3x3s2_dw_workspace_bytes(rows, c2, co2)) >= int(_lib.load().ma_gemm_tn_workspace_bytes(co2, 9 * c2, rows))
    dw2, db2 = torch.ones(co2, 9 * c2, device="cuda"), torch.ones(co2, device="cuda")  # += semantics: starts from ones
    K.conv2d_dw(dy_b.cuda(), act_b.cuda(), dw2, db2)
    rel = lambda a, w: float((a.cpu().double() - w.double()).abs().max() / w.double().abs().max())  # noqa: E731
    assert rel(dw2.view(co2, 3, 3, c2) - 1.0, wgt2.grad.permute(0, 2, 3, 1)) < 3e-5 and rel(db2 - 1.0, bias2.grad) < 3e-5


@pytest.mark.parametrize("m,k", [(1000, 2048), (10200, 768), (97, 512), (50000, 768)])
def test_input_gradient_product_with_layernorm_backward_epilogue(K, m, k):
    """ma_gemm_rows_train_bf16 mode 5 (round 4: da = du . W, the LayerNorm backward that consumes it and the next branch's dropout
    backward in ONE launch) against the two launches it replaces (dense_plain + layernorm_bwd_next): the same formulas with row sums
    taken in another order - g within 2e-6 of its scale, dgamma / dbeta (per-workgroup partials summed) within 2e-5, the emitted bf16
    dy_next equal except where a float32 last-digit difference crosses a bf16 rounding boundary (<= 1 bf16 ulp, < 0.5 % of entries),
    identical dropout zeros.  With and without a row scale / a next branch; M not a multiple of the 48- / 64-row tile."""
    from mindaudio_amd import _lib

    lib = _lib.load()
    g_ = torch.Generator().manual_seed(7 + m + k)
    d, p, seed = 256, 0.1, 4242
    st = torch.cuda.current_stream().cuda_stream

    def pack(w):
        n, kk = w.shape
        pieces = int(lib.ma_pack_item_pieces(1, n, kk))
        out = torch.empty(pieces * 16, dtype=torch.uint8, device="cuda")
        items = (_lib.PackItem * 1)(_lib.PackItem(w.data_ptr(), out.data_ptr(), w.stride(0), n, kk, 1, 0))
        d_items = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).cuda()
        d_map = torch.zeros((pieces + 255) // 256, dtype=torch.int32, device="cuda")
        _lib.check(lib.ma_pack_batch_bf16(d_items.data_ptr(), d_map.data_ptr(), d_map.numel(), st), "pack")
        return out

    du = bf(torch.randn(m, k, generator=g_)).cuda()
    wt = bf(torch.randn(d, k, generator=g_) / (k ** 0.5)).cuda()     # (256, k): the transposed weight of the layer
    x = torch.randn(m, d, generator=g_).cuda() * 2 + 0.3
    gamma = (1 + 0.1 * torch.randn(d, generator=g_)).cuda()
    g0 = torch.randn(m, d, generator=g_).cuda()
    rs = (torch.rand(m, generator=g_) > 0.2).float().cuda()
    wp = pack(wt)
    for row_scale, nxt in ((None, (0.5, p, seed, 9, None)), (rs, (1.0, p, seed, 10, rs)), (None, None)):
        g_ref, dg_ref, db_ref = g0.clone(), torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
        da = K.dense_plain(du, wp, d, k)
        if nxt is None:
            K.layernorm_bwd(x, gamma, da, g_ref, dg_ref, db_ref, row_scale=row_scale)
            dn_ref = None
        else:
            _, dn_ref = K.layernorm_bwd_next(x, gamma, da, g_ref, dg_ref, db_ref, nxt, row_scale=row_scale)
        g_new = g0.clone()
        parts = torch.full((K.rows_train_parts(m) * 512,), float("nan"), device="cuda")
        dn = K.dense_lnbwd(du, wp, k, x, gamma, g_new, parts, nxt=nxt, row_scale=row_scale)
        torch.cuda.synchronize()
        scale = float(g_ref.abs().max())
        assert float((g_new - g_ref).abs().max()) <= 2e-6 * scale + 1e-6
        pv = parts.view(-1, 512).double().sum(0)
        assert bool(torch.isfinite(pv).all())
        assert float((pv[:256] - dg_ref.double()).abs().max()) <= 2e-5 * float(dg_ref.abs().max()) + 1e-5
        assert float((pv[256:] - db_ref.double()).abs().max()) <= 2e-5 * float(db_ref.abs().max()) + 1e-5
        if nxt is None:
            assert dn is None
        else:
            a_, b_ = dn.float(), dn_ref.float()
            assert torch.equal(a_ == 0, b_ == 0)
            diff = (a_ - b_).abs()
            assert float((diff / b_.abs().clamp(min=1e-3)).max()) <= 1.0 / 64  # one bf16 ulp (2^-7 relative at most)
            assert float((diff > 0).float().mean()) < 5e-3


# ---- per-row gradient checks of the attention kernels (tests/attention_cases.py) ----------------------------------------------------
def _rows_of(t, name):
    return t.reshape(1, -1) if name in ("du", "dbv") else t


def _check_rows(tag, got, got32, ref, model, names, where):
    """Every gradient, row by row (du / dv as one row each), against float64 autograd: the bf16 kernel's worst row within
    GRAD_FACTOR x the rounded reference's worst row, the float32 kernel's within X32_ROW_TOL.  Prints the figures, then asserts."""
    GRAD_FACTOR, X32_ROW_TOL, worst = AC.GRAD_FACTOR, AC.X32_ROW_TOL, AC.worst
    bad = []
    for name in names:
        r = _rows_of(ref[name], name)
        e_k, at = worst(_rows_of(got[name], name), r)
        e_m, _ = worst(_rows_of(model[name], name), r)
        e_x, at_x = worst(_rows_of(got32[name], name), r)
        print("ROWS %s %-4s kernel %.2e (row %d = %s, |ref row| %.2e)  model %.2e  x32 %.2e (row %d)"
              % (tag, name, e_k, at, where(name, at), float(r[at].norm()), e_m, e_x, at_x))
        if not e_k <= GRAD_FACTOR * e_m:
            bad.append("%s: bf16 worst row %d (%s) %.3e > %g x model %.3e" % (name, at, where(name, at), e_k, GRAD_FACTOR, e_m))
        if not e_x <= X32_ROW_TOL:
            bad.append("%s: x32 worst row %d (%s) %.3e > %g" % (name, at_x, where(name, at_x), e_x, X32_ROW_TOL))
    assert not bad, "%s: %s" % (tag, "; ".join(bad))


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("b,t,h", AC.RELPOS_GRAD_SHAPES)
def test_attention_backward_rows(K, b, t, h, chunked):
    """ma_relpos_attention_bwd_bf16 / _x32 and their (B, T, T)-mask forms, per ROW: lens = [t, t - 37, 1] (a one-frame utterance next
    to a full one), q / k / v scaled so that a row has a few effective keys - one wrong key moves its row by O(1) - and dpos, du, dv
    preset (the kernels add to them).  The measured figures are in the module docstring.
    """
    from mindaudio_amd.train import kernels_x32 as X

    inp = AC.relpos_grad_inputs(b, t, h, chunked)
    ref, model = AC.relpos_float64(inp), AC.rounded_reference_relpos(inp)
    dm = h * 64
    qkv, pos, u, v, mask, dctx = (inp[n].cuda() for n in ("qkv", "pos", "u", "v", "mask", "dctx"))

    def run(fwd, bwd, cast):
        ctx, lse = fwd(cast(qkv), cast(pos), u, v, mask, b, t, heads=h)
        dpos, du, dv = inp["dpos0"].clone().cuda(), inp["du0"].clone().cuda(), inp["dv0"].clone().cuda()
        dqkv = bwd(cast(qkv), cast(pos), u, v, mask, ctx, cast(dctx), lse, b, t, dpos, du, dv, heads=h)
        sub = lambda buf, name: buf.double().cpu() - inp[name].double()  # noqa: E731  (what the kernel added)
        return dict(dq=dqkv[:, :dm], dk=dqkv[:, dm:2 * dm], dv=dqkv[:, 2 * dm:], dpos=sub(dpos, "dpos0"), du=sub(du, "du0"),
                    dbv=sub(dv, "dv0"))

    got = run(K.attention_fwd, K.attention_bwd, lambda x: x)
    got32 = run(X.attention_fwd, X.attention_bwd, lambda x: x.float())
    lens = inp["lens"].tolist()
    where = lambda name, r: ("t %d" % r if name == "dpos" else "-" if name in ("du", "dbv")  # noqa: E731
                             else "utterance %d of length %d, t %d" % (r // t, lens[r // t], r % t))
    _check_rows("relpos b%d t%d h%d %s" % (b, t, h, "chunk" if chunked else "pad"), got, got32, ref, model,
                ("dq", "dk", "dv", "dpos", "du", "dbv"), where)


@pytest.mark.parametrize("lq,lk,mode", AC.DECODER_GRAD_SHAPES)
def test_decoder_attention_backward_rows(K, lq, lk, mode):
    """ma_mha_small_bwd_bf16 / _x32 per ROW, the keys scaled by 8 (a few effective keys per row): one query and one key; the last
    key count of the LDS-staged matrix-core form (320) and the first beyond it (321), with two and three query tiles; 64 = two full
    tiles and 97 under the label mask.  The measured figures are in the module docstring.
    """
    from mindaudio_amd.train import kernels_x32 as X

    inp = AC.decoder_grad_inputs(lq, lk, mode)
    ref, model = AC.decoder_float64(inp), AC.rounded_reference_decoder(inp)
    b, h, scale = inp["b"], inp["heads"], inp["scale"]
    q, k, v, dctx = (inp[n].cuda() for n in ("q", "k", "v", "dctx"))
    mask = inp["mask"].cuda() if inp["mask"] is not None else None

    def run(mod, cast):
        ctx, probs = mod.mha_small_fwd(cast(q), cast(k), cast(v), mask, mode, b, lq, lk, scale, h, 64)
        dq, dk_, dv = (torch.empty_like(cast(x)) for x in (q, k, v))
        mod.mha_small_bwd(cast(q), cast(k), cast(v), probs, ctx, cast(dctx), b, lq, lk, scale, dq, dk_, dv, h, 64)
        return dict(dq=dq, dk=dk_, dv=dv)

    got, got32 = run(K, lambda x: x), run(X, lambda x: x.float())
    where = lambda name, r: "batch %d, %s %d" % ((r // lq, "query", r % lq) if name == "dq" else (r // lk, "key", r % lk))  # noqa: E731
    _check_rows("decoder lq%d lk%d mode%d" % (lq, lk, mode), got, got32, ref, model, ("dq", "dk", "dv"), where)
