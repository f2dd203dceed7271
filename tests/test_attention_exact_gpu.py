"""The attention forwards on one-hot inputs (tests/attention_cases.py): every query's softmax selects ONE key by construction, with an
off-target mass <= 2^-14, so the bf16 context row EQUALS the selected V row bit for bit - no tolerance stands between a kernel and
the question which key, head, batch, pos row or mask cell it used.  Lengths sit on both sides of every tile boundary of
relpos_attention_kernel (16-key fragments, 64-key tiles, the switch to the 8-wave 128-row kernel at (T - 1) % 128 >= 96) and of
mha_small_fwd (32-row query tiles, the LDS-staged / matrix-core limit of 320 keys, the 1088-key maximum); an utterance of length 1
runs next to a full one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available()
    from mindaudio_amd import ops
    from mindaudio_amd.train import kernels, kernels_x32

    return ops, kernels, kernels_x32


def bits(x):
    return x.contiguous().view(torch.int16)


def assert_rows_equal(got, want, case, variant, entry):
    """bf16 equality of whole tensors; on failure names the first wrong (batch, query) row."""
    got = got.cpu()
    if torch.equal(bits(got), bits(want)):
        return
    bad = torch.nonzero((bits(got) != bits(want)).any(1))[:, 0]
    r = int(bad[0])
    raise AssertionError("%s %s/%s/%s secondary=%s: %d of %d context rows differ from the selected V row, first (b, i) = (%d, %d), "
                         "lens %s" % (entry, case.perm, case.carrier, variant, case.secondary, bad.numel(), got.shape[0],
                                      r // case.T_q, r % case.T_q, case.lens))


def assert_lse(lse, want, what):
    err = float((lse.double().cpu() - want).abs().max())
    assert err <= 1e-3, (what, err)


@pytest.mark.parametrize("b,T,heads", AC.RELPOS_SHAPES)
def test_relpos_forward_selects_exactly(mods, b, T, heads):
    """ops.relpos_attention, the training forward (bf16) and the float32 forward, each in its (B, T) and (B, T, T) mask form: three
    permutations x three carriers, without and with secondary keys (padding mask; every primary hidden by the padding mask; the
    primaries of two queries in three hidden by single cells of the per-(query, key) mask)."""
    ops, K, X = mods
    for case in AC.relpos_selector_cases(b, T, heads):
        qkv, pos = case.qkv().cuda(), case.rows("pos").cuda()
        u, v = case.u.float().cuda(), case.v.float().cuda()
        for variant in case.variants():
            want, lse64, _, _ = case.expected(variant)
            mask = case.mask(variant)
            mask = mask.cuda() if mask is not None else None
            what = (case.perm, case.carrier, variant, case.secondary)
            assert_rows_equal(ops.relpos_attention(qkv, pos, u, v, mask, b, T, heads=heads), want, case, variant, "ops.relpos_attention")
            ctx, lse = K.attention_fwd(qkv, pos, u, v, mask, b, T, heads=heads)
            assert_rows_equal(ctx, want, case, variant, "K.attention_fwd")
            assert_lse(lse, lse64, ("K",) + what)
            ctx32, lse32 = X.attention_fwd(qkv.float(), pos.float(), u, v, mask, b, T, heads=heads)
            err = float((ctx32.double().cpu() - want.double()).abs().max())
            assert err <= AC.CTX_TOL, (("X",) + what, err)
            assert_lse(lse32, lse64, ("X",) + what)


@pytest.mark.parametrize("T", [17, 97, 129])
def test_relpos_forward_strided_views(mods, T):
    """qkv as a column slice of a wider buffer and out= as a column slice of another: the leading dimensions are not the widths, and
    what lies beside the output columns stays untouched."""
    ops, K, X = mods
    b, heads = 3, 4
    case = AC.selector_case(b, T, T, heads, AC.relpos_lens(b, T), "stride", "k+bias", AC.RELPOS_AMPLITUDE, secondary=True)
    dm = case.dm
    wide_in = torch.full((b * T, 3 * dm + 128), 3.0, dtype=torch.bfloat16, device="cuda")
    wide_in[:, 64:64 + 3 * dm] = case.qkv().cuda()
    wide_pos = torch.full((T, dm + 64), -3.0, dtype=torch.bfloat16, device="cuda")
    wide_pos[:, :dm] = case.rows("pos").cuda()
    u, v = case.u.float().cuda(), case.v.float().cuda()
    for variant in case.variants():
        want = case.expected(variant)[0]
        wide_out = torch.full((b * T, dm + 128), 7.0, dtype=torch.bfloat16, device="cuda")
        out = wide_out[:, 64:64 + dm]
        got = ops.relpos_attention(wide_in[:, 64:64 + 3 * dm], wide_pos[:, :dm], u, v, case.mask(variant).cuda(), b, T, heads=heads, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert_rows_equal(out, want, case, variant, "ops.relpos_attention(out=)")
        assert bool((wide_out[:, :64] == 7.0).all()) and bool((wide_out[:, 64 + dm:] == 7.0).all())
        ctx, _ = K.attention_fwd(wide_in[:, 64:64 + 3 * dm], wide_pos[:, :dm], u, v, case.mask(variant).cuda(), b, T, heads=heads)
        assert_rows_equal(ctx, want, case, variant, "K.attention_fwd(views)")


MODE_OF = {"nomask": 0, "pad": 1, "pad_sec": 1, "cell": 2}


def check_probs(probs, case, variant, entry):
    """>= 1 - 2^-13 at the selected key, <= 2^-13 at every other one - the masked ones (the reference gives exp(-10000) = 0) among them."""
    sel = case.selected(variant)
    p = probs.double().cpu()
    idx = sel[:, None, :, None].expand(-1, case.heads, -1, 1)
    at = torch.gather(p, 3, idx)
    assert float(at.min()) >= 1 - AC.PROB_TOL, (entry, variant, float(at.min()))
    rest = p.scatter(3, idx, 0.0)
    assert float(rest.max()) <= AC.PROB_TOL, (entry, variant, float(rest.max()))
    m = case.mask(variant)
    if m is not None:
        kb = torch.arange(case.b) // case.kv_group
        hidden = (m[kb][:, None, None, :] if m.dim() == 2 else m[:, None]) == 0
        assert float((p * hidden).max()) <= AC.PROB_TOL, (entry, variant)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("lq,lk", AC.DECODER_SHAPES)
def test_decoder_forward_selects_exactly(mods, lq, lk, mode):
    """ma_mha_small_fwd (bf16: the matrix-core form up to 320 keys, the score-rows-in-LDS form beyond), its grouped form (query batch b
    reads the keys of batch b // 2) and the float32 form, mask modes 0 (none), 1 (B, 1, Lk) and 2 (B, Lq, Lk)."""
    _, K, X = mods
    b, h, scale = AC.DECODER_B, 4, 1.0 / AC.DK
    ran = 0
    for group in (1, 2):
        for case in AC.decoder_selector_cases(lq, lk, kv_group=group):
            q, k, v = (case.rows(n).cuda() for n in ("q", "k", "val"))
            for variant in case.variants():
                if MODE_OF[variant] != mode:
                    continue
                want = case.expected(variant)[0]
                mask = case.mask(variant)
                mask = mask.cuda() if mask is not None else None
                if group == 2:
                    ctx, probs = K.mha_small_fwd_grouped(q, k, v, mask, mode, b, lq, lk, scale, 2, h, AC.DK)
                    assert_rows_equal(ctx, want, case, variant, "mha_small_fwd_grouped")
                    check_probs(probs, case, variant, "grouped")
                else:
                    ctx, probs = K.mha_small_fwd(q, k, v, mask, mode, b, lq, lk, scale, h, AC.DK)
                    assert_rows_equal(ctx, want, case, variant, "mha_small_fwd")
                    check_probs(probs, case, variant, "bf16")
                    ctx32, probs32 = X.mha_small_fwd(q.float(), k.float(), v.float(), mask, mode, b, lq, lk, scale, h, AC.DK)
                    err = float((ctx32.double().cpu() - want.double()).abs().max())
                    assert err <= AC.CTX_TOL, ("x32", case.perm, variant, err)
                    check_probs(probs32, case, variant, "x32")
                ran += 1
    assert ran >= 6
