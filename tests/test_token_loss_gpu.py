"""The CTC kernels (csrc/ctc.hip), the label-smoothing loss and the embedding kernels (csrc/decoder_kernels.hip) against the float64
references of tests/token_loss_cases.py, per utterance and per row, at the kernels' own edges: the 4-step emission prefetch ring
(tlen 1 .. 9), the carries between 64-state chunks (states 63 / 64 / 65 .. 254 in the 4-chunk form, .. 446 in the 7-chunk form),
adjacent and non-adjacent repeats, a label that equals the blank, blanks other than 0, the feasibility boundary, hlens > T, and the
scalar fallbacks of ctc_lse_kernel / ctc_dlogits_kernel (ld % 4 != 0, an unaligned base, V > 5120); vocabularies of 2 .. 4233 columns
on both sides of the label-smoothing kernel's 256-column stride; the embedding backward's 1024-row stages, 8-row walk, runs of one
token and one-writer-per-token rule, bit for bit on integer-valued inputs.  test_token_loss_cases_cpu.py shows that these checks, with
these tolerances, reject each of eleven planted defects.

What a float32 gradient row may be off by is 4 x what float32 CPU torch is off by on the same case (computed here, never taken from
the kernels), with a floor of 8 * 2^-24 * max(1, nll) (CTC) or 8 * 2^-24 * max(1, max |logit|) (label smoothing); a bf16 row one bf16
ulp per element more.

Measured on an MI355X (worst gradient row per utterance, ||got - want||: kernel / float32 CPU torch, against the same float64 reference;
each test prints its figures with -s):
  CTC float32 gradient (ma_ctc_loss_grad_x32)                                     kernel    torch    allowed (4 x torch | floor)
    ring         tlen 9, 3 labels (nll 22, grad_scale 0.5)                        1.5e-06   1.7e-06  6.6e-06
    chunk4       U = 31, one alignment (nll 158, grad_scale 2)                    3.1e-05   5.1e-05  2.0e-04
    chunk4       U = 127, one alignment (nll 633)                                 3.7e-04   3.8e-04  1.5e-03
    chunk7       U = 128 (nll 616)                                                4.8e-04   6.0e-04  2.4e-03
    chunk7       U = 223, one alignment (nll 1120)                                1.5e-03   1.4e-03  5.6e-03
    feasibility  U = 64, 3 adjacent repeats, 67 frames                            6.1e-05   5.4e-05  2.2e-04
    uniform66    U = 66, T = 78 against the integer counts                        6.7e-05   5.4e-05  2.2e-04
    uniform223   U = 223, T = 229 against the integer counts (nll 434)            8.5e-04   7.2e-04  2.9e-03
    the worst ratio kernel / allowed over all 22 cases is 0.34 (chunk4); the addressing cases lie between 0.11 and 0.30
  CTC bf16 gradient (ma_ctc_loss_grad_f32): 3e-03 .. 5.5e-03 per row at grad_scale 2 (rounding: one bf16 ulp per element allows
    7.8e-03 ||want_row||); the worst ratio kernel / allowed is 0.78
  per-utterance nll: all three entry points within 1.9e-06 relative (uniform223; 1e-05 allowed) - float32 torch is off by the same
    1.9e-06 there, 3.7e-07 on chunk7, 1e-07 elsewhere; ops.ctc_loss and the gradient path agreed bit for bit on every case
  label smoothing, KL sum (kernel / float32 torch / allowed rows * 2^-20 * max(1, |want|)):
    V 4233, 130 rows, smoothing 0.5   4.1e-05 / 2.0e-05 / 3.6e-02        V 1000, 65 rows   7.8e-06 / 7.8e-06 / 1.5e-02
    shift40 (V 4233, 5 rows, +40)     3.5e-06 / 1.5e-06 / 8.0e-05        ties              7.1e-07 / 7.1e-07 / 3.2e-05
    (sum_logp = sl - V * lse under the +40 shift costs a factor 2.2 against torch, far inside the bound)
  label smoothing, float32 gradient rows: worst ratio kernel / allowed 0.08 (ties: 1.2e-07 against torch's 4.4e-08, floor 1.6e-06);
    row sums within 0.69 of V * 2^-24 * scale (V = 7; 0.04 and less from V = 257 on); bf16 rows within 0.90 of their bound
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import token_loss_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available()
    from mindaudio_amd import _lib, ops
    from mindaudio_amd.train import kernels, kernels_x32

    return ops, kernels, kernels_x32, _lib


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


# ---- CTC ----------------------------------------------------------------------------------------------------------------------------
def batch_loss(per, B):
    """ctc_reduce_kernel's arithmetic: the finite losses added in float32 in batch order, / B."""
    s = np.float32(0.0)
    for v in per.cpu().numpy():
        s = np.float32(s + (np.float32(0.0) if np.isinf(v) else v))
    return float(np.float32(s / np.float32(B)))


@pytest.mark.parametrize("name", list(TC.ctc_cases()))
def test_ctc_per_utterance_and_per_row(mods, name):
    ops, K, X, _ = mods
    case, ref = TC.ctc_cases()[name], TC.ctc_reference(name)
    logits = case.device_logits("cuda")
    assert logits.stride(0) == case.ld and (logits.data_ptr() % 16 != 0) == bool(case.offset)
    ys, hlens, ylens = i32(case.ys), i32(case.hlens), i32(case.ylens)
    loss16, per16, d16 = K.ctc_loss_grad(logits, case.V, case.B, case.T, ys, hlens, ylens, case.grad_scale, blank=case.blank)
    loss32, per32, d32 = X.ctc_loss_grad(logits, case.V, case.B, case.T, ys, hlens, ylens, case.grad_scale, blank=case.blank)
    loss_f, per_f = ops.ctc_loss(logits, case.B, case.T, ys, hlens, ylens, blank=case.blank)
    torch.cuda.synchronize()
    print("\n%s: ops.ctc_loss and the gradient path agree bit for bit: %s" % (name, torch.equal(per_f, per32) and torch.equal(per16, per32)))
    for what, dlog, bf16 in (("bf16", d16, True), ("float32", d32, False)):
        assert tuple(dlog.shape) == (case.B * case.T, case.ld)
        full = dlog.float().cpu().view(case.B, case.T, case.ld)
        assert not bool(full[..., case.V:].any()), (what, "pad columns")
        per = per16 if bf16 else per32
        m = TC.ctc_margins(case, ref, per, full, bf16=bf16)
        err = TC.row_err(full[..., :case.V], ref.grad).max(dim=1).values
        print("  %-7s worst row error per utterance / float32 torch's: %s" % (what, " ".join(
            "%.1e/%.1e" % (e, y) for e, y in zip(err.tolist(), ref.yard.tolist()))))
        print("  %-7s margins %s   (nll: float32 torch is off by %.1e relative)" % (what, m, ref.yard_nll))
        assert m["exact"] == 0.0, (what, "rows past the length / utterances without an alignment must be exactly zero")
        assert m["nll"] <= 1.0, (what, m)
        assert m["row"] <= 1.0, (what, m)
    m = TC.ctc_margins(case, ref, per_f, ref.grad)
    assert m["nll"] <= 1.0, ("ops.ctc_loss", m)
    for loss, per in ((loss16, per16), (loss32, per32), (loss_f, per_f)):
        assert float(loss) == batch_loss(per, case.B)
        assert bool((torch.isinf(per.cpu()) == torch.isinf(ref.nll)).all())


def test_ctc_host_refusals(mods):
    ops, K, X, _lib = mods
    refused = (NotImplementedError, _lib.MindaudioAmdError)
    one = i32([1])
    wide = torch.zeros(1, 15361, device="cuda")  # 15361 * 4 bytes > 60 KiB of LDS for the occupancies
    for mod in (K, X):
        with pytest.raises(refused):
            mod.ctc_loss_grad(wide, 15361, 1, 1, i32([[1]]), one, one, 1.0)
    small = torch.zeros(4, 8, device="cuda")
    long_ys = torch.ones(1, 224, dtype=torch.int32, device="cuda")  # 449 states
    for mod in (K, X):
        with pytest.raises(refused):
            mod.ctc_loss_grad(small, 8, 1, 4, long_ys, i32([4]), one, 1.0)
    with pytest.raises(refused):
        ops.ctc_loss(small, 1, 4, long_ys, i32([4]), one)
    torch.cuda.synchronize()


# ---- label smoothing ----------------------------------------------------------------------------------------------------------------
LSM = {c.name: c for c in TC.lsm_cases()}


@pytest.mark.parametrize("name", list(LSM))
def test_label_smoothing_stats_and_rows(mods, name):
    _, K, X, _ = mods
    case = LSM[name]
    ref = TC.LsmReference(case)
    logits = case.device_logits("cuda")
    assert logits.stride(0) == case.ld
    target, mask = i32(case.target), case.mask.cuda()
    for what, mod, bf16 in (("bf16", K, True), ("float32", X, False)):
        stats, dlog = mod.label_smoothing_loss_grad(logits, case.V, target, mask, case.smoothing, case.grad_scale,
                                                    normalize_length=case.normalize_length)
        torch.cuda.synchronize()
        assert tuple(dlog.shape) == (case.rows, case.ld)
        full = dlog.float().cpu()
        assert not bool(full[:, case.V:].any()), (what, "pad columns")
        m = TC.lsm_margins(case, ref, stats, full, bf16=bf16)
        err = float(TC.row_err(full[:, :case.V], ref.grad).max())
        print("\n%s %s: KL sum off by %.2e (float32 torch %.2e, allowed %.2e); worst row %.2e (float32 torch %.2e, allowed %.2e%s); %s"
              % (name, what, abs(float(stats[0]) - float(ref.stats[0])), ref.yard_kl, ref.kl_tol, err, ref.yard, ref.bound,
                 " + bf16 ulp" if bf16 else "", m))
        assert m["exact"] == 0.0, (what, stats.tolist(), ref.stats.tolist())
        assert m["kl"] <= 1.0, (what, m)
        assert m["row"] <= 1.0, (what, m)
        assert m.get("rowsum", 0.0) <= 1.0, (what, m)
        if name == "all_masked":
            assert not bool(stats.any()) and not bool(full.any())


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L,D,V", TC.EMBED_FWD)
def test_embedding_forward_is_exact(mods, rows, L, D, V):
    _, K, _, _ = mods
    c = TC.embed_forward_case(rows, L, D, V)
    out = K.embed_posenc(c["tokens"].cuda(), c["table"].float().cuda(), c["pe"].float().cuda(), L, c["xscale"], 0.0, 0, 0)
    assert torch.equal(out.cpu(), TC.embed_forward_expected(c).float())


@pytest.mark.parametrize("rows,L,D,V", TC.EMBED_FWD)
def test_embedding_dropout_forward_and_backward_share_one_mask(mods, rows, L, D, V):
    _, K, _, _ = mods
    c = TC.embed_forward_case(rows, L, D, V, positive=True)
    tok, table, pe = c["tokens"].cuda(), c["table"].float().cuda(), c["pe"].float().cuda()
    want = TC.embed_forward_expected(c).float()
    seed, salt = 1234, 77
    out = K.embed_posenc(tok, table, pe, L, c["xscale"], 0.5, seed, salt).cpu()
    kept = out != 0
    assert torch.equal(out, torch.where(kept, 2.0 * want, torch.zeros_like(want)))  # every element 0 or 2 x expected
    n = rows * D
    assert abs(float((~kept).float().mean()) - 0.5) <= 4.0 * (0.25 / n) ** 0.5
    other = K.embed_posenc(tok, table, pe, L, c["xscale"], 0.5, seed, salt + 1).cpu() != 0
    assert not torch.equal(other, kept)
    assert torch.equal(K.embed_posenc(tok, table, pe, L, c["xscale"], 0.5, seed, salt).cpu(), out)
    # the backward under the same (seed, salt) drops what the forward dropped
    g = torch.Generator().manual_seed(rows + D)
    bc = dict(rows=rows, D=D, V=V, tokens=c["tokens"], g=TC._ints(g, (rows, D), -8, 8), dtable0=TC._ints(g, (V, D), -16, 16),
              xscale=c["xscale"])
    keep = (torch.rand(rows, generator=g) < 2.0 / 3.0).float()
    for row_keep in (None, keep):
        dtable = bc["dtable0"].float().cuda()
        K.embed_bwd(tok, bc["g"].float().cuda(), dtable, c["xscale"], 0.5, seed, salt,
                    row_keep=row_keep.cuda() if row_keep is not None else None)
        assert torch.equal(dtable.cpu(), TC.embed_backward_expected(bc, row_keep, factor=2 * kept.long()).float())


@pytest.mark.parametrize("D", TC.EMBED_BWD_D)
def test_embedding_backward_equals_index_add(mods, D):
    _, K, _, _ = mods
    for pattern in TC.EMBED_PATTERNS:
        for rows in TC.EMBED_BWD_ROWS:
            c = TC.embed_backward_case(pattern, rows, D)
            tok, g = c["tokens"].cuda(), c["g"].float().cuda()
            for row_keep in (None, c["keep"]):
                dtable = c["dtable0"].float().cuda()
                K.embed_bwd(tok, g, dtable, c["xscale"], 0.0, 5, 7, row_keep=row_keep.cuda() if row_keep is not None else None)
                want = TC.embed_backward_expected(c, row_keep).float()
                got = dtable.cpu()
                if not torch.equal(got, want):
                    bad = torch.nonzero((got != want).any(1))[:, 0]
                    raise AssertionError("%s rows %d D %d row_keep %s: %d table rows differ, first token id %d"
                                         % (pattern, rows, D, row_keep is not None, bad.numel(), int(bad[0])))
    # nothing contributes where every row is skipped
    dtable = c["dtable0"].float().cuda()
    K.embed_bwd(tok, g, dtable, c["xscale"], 0.0, 5, 7, row_keep=torch.zeros(c["rows"], device="cuda"))
    assert torch.equal(dtable.cpu(), c["dtable0"].float())


def test_embedding_backward_refuses_more_than_1024_features(mods):
    """embed_bwd_kernel<4> covers 4 x 256 features: D = 1280 returned MA_OK and left features >= 1024 without a gradient."""
    _, K, _, _lib = mods
    rows, D, V = 9, 1280, 7
    tok = torch.arange(rows, dtype=torch.int32, device="cuda") % V
    g = torch.ones(rows, D, device="cuda")
    for row_keep in (None, torch.ones(rows, device="cuda")):
        dtable = torch.zeros(V, D, device="cuda")
        with pytest.raises((NotImplementedError, _lib.MindaudioAmdError)):
            K.embed_bwd(tok, g, dtable, 1.0, 0.0, 0, 0, row_keep=row_keep)
        assert not bool(dtable.any())
