"""The builders and comparators of tests/attention_cases.py, without a device: every selector case the GPU tests run meets the one-hot
condition, the float64 references agree with each other, and the per-row comparator SEES a single wrong row, a single dropped key and
a mask shifted by one column - where the whole-tensor norm it replaces does not."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_cases as AC  # noqa: E402


@pytest.mark.parametrize("b,T,heads", AC.RELPOS_SHAPES)
def test_relpos_selector_cases_are_one_hot(b, T, heads):
    n = 0
    for case in AC.relpos_selector_cases(b, T, heads):  # (the builder asserts exactness, distinct V rows and the off-target mass)
        for variant in case.variants():
            ctx, lse, sel, off = case.expected(variant)
            assert float(off.max()) <= AC.OFF_MASS
            assert bool((sel < torch.tensor(case.lens)[:, None]).all())
            # the float64 context is within 2^-12 of the selected V row: a sixteenth of half a bf16 ulp in [1, 2)
            assert float((case.context64(case.mask(variant)) - ctx.double()).abs().max()) <= AC.CTX_TOL
            n += 1
        if case.secondary and T >= 2:
            assert bool((case.selected("pad_sec")[0] != case.pri[0]).all())          # the full utterance: every primary hidden
            cell = case.selected("cell") != case.pri
            assert bool(cell[0].any()) and (T < 3 or not bool(cell[0].all()))       # some queries of a tile, not all
    assert n == 54


def test_permutations_reach_every_key_and_scatter():
    for n in (1, 2, 17, 97, 301):
        for name in AC.PERMS:
            assert sorted(AC.permutation(name, n, n).tolist()) == list(range(n))
    assert AC.permutation("reversal", 301, 301)[0] == 300
    s = AC.permutation("stride", 301, 301)
    assert len({int(x) // 64 for x in s[:16]}) >= 4  # one 16-query fragment reads from at least four key tiles


@pytest.mark.parametrize("lq,lk", AC.DECODER_SHAPES)
def test_decoder_selector_cases_are_one_hot(lq, lk):
    for group in (1, 2):
        for case in AC.decoder_selector_cases(lq, lk, kv_group=group):
            for variant in case.variants():
                ctx, lse, sel, off = case.expected(variant)
                assert float(off.max()) <= AC.OFF_MASS
                probs = torch.softmax(case.scores(variant), -1)
                at = torch.gather(probs, 3, sel[:, None, :, None].expand(-1, 4, -1, 1))
                assert float(at.min()) >= 1 - AC.PROB_TOL


def test_rowwise_err_floors_the_zero_rows():
    ref = torch.zeros(5, 8, dtype=torch.float64)
    ref[0], ref[1], ref[2] = 1.0, 2.0, 4.0
    got = ref.clone()
    got[3, 0] = 2.0 ** -6 * ref[1].norm() * 0.5  # a structurally zero row, wrong by half the floor
    got[2, 0] += 0.4
    err, at = AC.rowwise_err(got, ref)
    assert AC.row_floor(ref) == pytest.approx(2.0 ** -6 * float(ref[1].norm()))
    assert err[3] == pytest.approx(0.5) and at == 3 and err[2] == pytest.approx(0.4 / float(ref[2].norm()))


# ---- the gradient references ------------------------------------------------------------------------------------------------------
GRADS = ("dq", "dk", "dv", "dpos", "du", "dbv")


def _relpos_bounds(inp):
    ref = AC.relpos_float64(inp)
    model = AC.rounded_reference_relpos(inp)
    bound = {}
    for name in GRADS:
        r, m = (ref[name].reshape(1, -1), model[name].reshape(1, -1)) if name in ("du", "dbv") else (ref[name], model[name])
        bound[name] = AC.GRAD_FACTOR * AC.worst(m, r)[0]
    return ref, model, bound


@pytest.mark.parametrize("b,T,heads", AC.RELPOS_GRAD_SHAPES)
@pytest.mark.parametrize("chunked", [False, True])
def test_relpos_rounded_reference_is_a_bf16_model(b, T, heads, chunked):
    """The rounded model differs from float64 autograd by bf16 rounding and nothing else: not identical to it, and its worst row (a
    few per cent where rounding q + u moves a sharp softmax) leaves the 4 x bound below 0.5 - half of what a zeroed row measures."""
    inp = AC.relpos_grad_inputs(b, T, heads, chunked)
    ref, model, bound = _relpos_bounds(inp)
    for name in GRADS:  # (T = 1: the softmax is 1, dv = dctx exactly and the other gradients vanish)
        assert (0 < bound[name] or T == 1) and bound[name] < 0.5, (name, bound[name])
    # (bf16(q + u): 64 products of |q + u| ~ 2 rounded at 2^-9 with |k| ~ 1.6, over 8: the scores move by about 1e-2)
    assert float((model["lse"] - ref["lse"]).abs().max()) < 0.05


@pytest.mark.parametrize("lq,lk,mode", AC.DECODER_GRAD_SHAPES)
def test_decoder_rounded_reference_is_a_bf16_model(lq, lk, mode):
    inp = AC.decoder_grad_inputs(lq, lk, mode)
    ref, model = AC.decoder_float64(inp), AC.rounded_reference_decoder(inp)
    for name in ("dq", "dk", "dv"):
        e = AC.worst(model[name], ref[name])[0]
        assert (0 < e or lk == 1) and AC.GRAD_FACTOR * e < 0.5, (name, e)
    assert float((model["probs"] - ref["probs"]).abs().max()) < 1e-5


def test_rowwise_err_sees_what_the_whole_tensor_norm_misses():
    """(3, 65, 4) with the chunk mask.  Three errors of the kind a kernel makes in ONE place, applied to the float64 reference: each
    exceeds the bound the GPU test uses (4 x the rounded model's worst row)."""
    b, T, heads = 3, 65, 4
    inp = AC.relpos_grad_inputs(b, T, heads, True)
    ref, model, bound = _relpos_bounds(inp)
    # 1. the last row of the full utterance comes out zero
    for name in ("dq", "dk", "dv"):
        bad = ref[name].clone()
        bad[T - 1] = 0
        e, at = AC.worst(bad, ref[name])
        assert at == T - 1 and e == pytest.approx(1.0) and e > bound[name]
    bad = ref["dpos"].clone()
    bad[T - 1] = 0
    assert AC.worst(bad, ref["dpos"])[0] > bound["dpos"]
    # 2. one query row (the last of the last tile) loses its most probable key
    q, k, vv, p = AC._relpos_split(inp)
    i0 = T - 1
    s = torch.einsum("hd,jhd->hj", q[0, i0] + inp["u"].double(), k[0]) + torch.einsum("hd,jhd->hj", q[0, i0] + inp["v"].double(), p)
    s = s / 8.0 + (inp["mask"][0, i0] == 0).double() * AC.MASKED
    j0 = int(torch.softmax(s, -1).sum(0).argmax())
    dropped = inp["mask"].clone()
    dropped[0, i0, j0] = 0
    got = AC.relpos_float64(inp, dropped)
    e, at = AC.worst(got["dq"], ref["dq"])
    assert at == i0 and e > bound["dq"]
    for name in ("dk", "dv"):
        e, at = AC.worst(got[name], ref[name])
        assert e > bound[name], name
    # 3. one utterance's (B, T, T) mask is shifted by one column
    shifted = inp["mask"].clone()
    shifted[1] = torch.roll(shifted[1], 1, dims=-1)
    got = AC.relpos_float64(inp, shifted)
    for name in ("dq", "dk", "dv", "dpos"):
        e, at = AC.worst(got[name], ref[name])
        assert e > bound[name], name
        if name != "dpos":
            assert T <= at < 2 * T  # ... and it names a row of that utterance


def test_old_metric_passes_a_zeroed_row_at_64_by_255():
    """The gap this file closes: at (b, t) = (64, 255) - the case of test_attention_backward that runs more than three resident
    rounds of workgroups - an all-zero dq row moves ||got - want|| / ||want|| by about 1 / sqrt(16320) = 0.8 %, inside its 2e-2;
    per row it is an error of 1."""
    b, T, heads = 64, 255, 4
    g = torch.Generator().manual_seed(7 + T)
    lens = torch.randint(T // 2, T + 1, (b,), generator=g)
    lens[0] = T
    inp = AC.relpos_grad_inputs(b, T, heads, False, lens=lens.tolist(), qkv_scale=0.8)
    dq = []
    for b0 in range(0, b, 8):  # (dq of an utterance depends on that utterance alone: by slices of the batch)
        rows = slice(b0 * T, (b0 + 8) * T)
        part = dict(inp, b=8, qkv=inp["qkv"][rows], dctx=inp["dctx"][rows], mask=inp["mask"][b0:b0 + 8])
        dq.append(AC.relpos_float64(part)["dq"])
    want = torch.cat(dq).float()
    got = want.clone()
    got[b * T - 1] = 0  # the last row of the last tile of the last utterance
    assert AC.old_rel(got, want) < 2e-2
    assert AC.old_rel(got, want) == pytest.approx(1 / (b * T) ** 0.5, rel=0.5)
    e, at = AC.worst(got, want)
    assert at == b * T - 1 and e == pytest.approx(1.0)
    # (3, 255): a row wrong by half - 1.8 % of the whole tensor, also inside 2e-2
    small = want[:3 * T].clone()
    bad = small.clone()
    bad[3 * T - 1] *= 0.5
    assert AC.old_rel(bad, small) < 2e-2 and AC.worst(bad, small)[0] == pytest.approx(0.5)


def test_the_same_errors_change_a_selector_row_completely():
    """On a selector case the three errors replace a context row by ANOTHER V row (or by zeros): every comparison of the GPU test
    is an equality, so any of them fails it."""
    T = 65
    case = AC.selector_case(3, T, T, 4, AC.relpos_lens(3, T), "reversal", "k", AC.RELPOS_AMPLITUDE, secondary=True)
    want, _, sel, _ = case.expected("cell")
    bits = lambda x: x.to(torch.bfloat16).view(torch.int16)  # noqa: E731
    assert torch.equal(bits(case.context64(case.mask("cell"))), bits(want))
    # 1. a zeroed last row
    zero = want.clone()
    zero[T - 1] = 0
    assert bool((bits(zero)[T - 1] != bits(want)[T - 1]).all())
    # 2. query T - 1 of utterance 0 loses the key it selects: it now returns another key's V row
    m = case.mask("cell").clone()
    m[0, T - 1, sel[0, T - 1]] = 0
    got = case.context64(m)
    changed = (bits(got) != bits(want)).any(1)
    assert bool(changed[T - 1]) and int(changed.sum()) == 1
    assert float((got[T - 1] - want[T - 1].double()).abs().max()) >= 2.0 ** -7  # (a whole V quantum, not a rounding)
    # 3. utterance 1's mask shifted by one column: the hidden cell moves off the primary, the flagged queries return their primaries
    m = case.mask("cell").clone()
    m[1] = torch.roll(m[1], 1, dims=-1)
    changed = (bits(case.context64(m)) != bits(want)).any(1)
    assert int(changed[T:2 * T].sum()) >= T // 2 and not bool(changed[:T].any())
