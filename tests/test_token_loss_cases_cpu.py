"""The references, cases and comparators of tests/token_loss_cases.py, without a device: the CTC references agree with each other
and with a brute-force path sum, every case meets the condition its test rests on, and the checks of test_token_loss_gpu.py - with
the very tolerances that test uses - reject a float64 model of each operation that carries ONE planted defect, by a factor of ten or
more; two of the CTC defects are shown to pass the whole-tensor norm bound these tests replace."""
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import token_loss_cases as TC  # noqa: E402
from oracle import conformer_oracle as C  # noqa: E402

REJECT = 10.0


def worst(margins):
    return max(margins.values())


# ---- the references agree -----------------------------------------------------------------------------------------------------------
def brute_force(lp, target, blank):
    """-log of the summed probability of every length-T path that collapses (repeats, then blanks) to `target`, and their number."""
    T, V = lp.shape
    acc, n = 0.0, 0
    for path in itertools.product(range(V), repeat=T):
        collapsed = [s for s, prev in zip(path, (None,) + path[:-1]) if s != prev and s != blank]
        if collapsed == target:
            acc += math.exp(sum(float(lp[t, s]) for t, s in enumerate(path)))
            n += 1
    return (-math.log(acc) if n else math.inf), n


@pytest.mark.parametrize("blank", [0, 2, 3])
def test_ctc_references_against_brute_force_path_sum(blank):
    V, T = 4, 6
    labels = [v for v in range(V) if v != blank]
    targets = [[], [labels[0]], [labels[0], labels[1]], [labels[2], labels[2]], [labels[0], labels[0], labels[1]],
               [labels[1], labels[2], labels[1]], [labels[0], labels[0], labels[0], labels[0]]]
    logits = torch.randn(len(targets), T, V, generator=torch.Generator().manual_seed(5 + blank))
    ys = TC._pack(targets, 4)
    ylens = [len(t) for t in targets]
    for tlen in (6, 5, 3):
        hlens = [tlen] * len(targets)
        nll, grad = TC.ctc_float64(logits, ys, hlens, ylens, blank, 1.0)
        lp = torch.log_softmax(logits.double(), -1)
        for b, target in enumerate(targets):
            want, n = brute_force(lp[b, :tlen], target, blank)
            assert n == TC.count_alignments(target, tlen, blank)
            n_c, nll_c, _ = TC.ctc_counting(target, tlen, V, blank)
            assert n_c == n and (n == 0 or abs(nll_c - (tlen * math.log(V) - math.log(n))) < 1e-12)
            nll_m, grad_m = TC.ctc_model(logits[b], target, tlen, blank, 1.0)
            if n == 0:
                assert math.isinf(float(nll[b])) and math.isinf(nll_m) and not bool(grad[b].any()) and not bool(grad_m.any())
                continue
            assert abs(float(nll[b]) - want) < 1e-10 and abs(nll_m - want) < 1e-10
            assert float((grad[b] - grad_m).abs().max()) < 1e-12
            if n == 1:
                nll_s, grad_s = TC.ctc_single_alignment(logits[b], target, tlen, blank, 1.0)
                assert abs(nll_s - want) < 1e-10 and float((grad_s - grad[b]).abs().max()) < 1e-12


@pytest.mark.parametrize("name", ["uniform66", "uniform223"])
def test_ctc_counting_agrees_with_float64_torch(name):
    """Exact integer counts against float64 torch on all-zero logits: U = 0, (1, 1), adjacent repeats, a label that equals the blank,
    447 states."""
    case, ref = TC.ctc_cases()[name], TC.ctc_reference(name)
    nll, grad = TC.ctc_float64(case.logits, case.ys, case.hlens, case.ylens, case.blank, case.grad_scale)
    assert float((nll - ref.nll).abs().max()) < 1e-9
    assert float((grad - ref.grad).abs().max()) < 1e-11
    nll_m, grad_m = TC.ctc_model_batch(case)
    assert float((nll_m - ref.nll).abs().max()) < 1e-9 and float((grad_m - ref.grad).abs().max()) < 1e-11


@pytest.mark.parametrize("name", ["ring", "chunk4", "chunk7", "feasibility", "addr_V11_ld13_blank3", "addr_V5121_ld5124_blank5120"])
def test_ctc_model_and_closed_form_agree_with_float64_torch(name):
    case, ref = TC.ctc_cases()[name], TC.ctc_reference(name)
    nll_m, grad_m = TC.ctc_model_batch(case)
    assert bool((torch.isinf(nll_m) == torch.isinf(ref.nll)).all())
    fin = ~torch.isinf(ref.nll)
    assert float(((nll_m - ref.nll)[fin].abs() / ref.nll[fin].abs().clamp_min(1.0)).max()) < 1e-12
    assert float((grad_m - ref.grad).abs().max()) < 1e-10
    for b in case.single:
        nll_s, grad_s = TC.ctc_single_alignment(case.logits[b], case.labels(b), case.tlen(b), case.blank, case.grad_scale)
        assert abs(nll_s - float(ref.nll[b])) < 1e-12 * max(1.0, abs(nll_s))
        assert float((grad_s - ref.grad[b]).abs().max()) < 1e-10
    # a correct float64 model passes every check of the GPU test, in both output types
    for bf16 in (False, True):
        assert worst(TC.ctc_margins(case, ref, nll_m, grad_m, bf16=bf16)) <= 1e-3


def test_ctc_case_conditions():
    """Single-alignment utterances have N == 1, infeasible ones N == 0, every other one N >= 1; the lists hold what they promise."""
    cases = TC.ctc_cases()
    assert len(cases) == 6 + 16
    for case in cases.values():
        for b in range(case.B):
            n = TC.count_alignments(case.labels(b), case.tlen(b), case.blank)
            if b in case.single:
                assert n == 1, (case.name, b)
            elif b in case.infeasible:
                assert n == 0, (case.name, b)
            else:
                assert n >= 1 and (case.name != "feasibility"), (case.name, b)
    ring = cases["ring"]
    assert [ring.tlen(b) for b in range(ring.B)] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9] and ring.hlens[-1] > ring.T
    assert any(TC.adjacent_repeats(ring.labels(b)) for b in range(ring.B))
    c4, c7 = cases["chunk4"], cases["chunk7"]
    assert c4.Lmax == 127 and 2 * c4.Lmax + 1 <= 256 and c7.Lmax == 223 and 2 * c7.Lmax + 1 == 447
    assert len(c4.single) >= 2 and len(c7.single) >= 2 and c4.blank in c4.labels(5) and c7.blank in c7.labels(4)
    for case in (c4, c7):
        for b in range(case.B - 1):  # non-adjacent repeats everywhere
            assert len(set(case.labels(b))) < case.ylens[b]
    feas = cases["feasibility"]
    assert len(feas.single) == len(feas.infeasible) == len(TC.FEASIBILITY_PAIRS)
    assert sum(1 for c in cases.values() if c.offset) == 1
    assert {c.blank for c in cases.values() if c.name.startswith("addr_V11_")} == {0, 3, 10}


def test_label_smoothing_reference_agrees_with_the_oracle():
    for case in TC.lsm_cases():
        stats, kl, grad = TC.lsm_float64(case.logits, case.target, case.mask, case.smoothing, case.grad_scale, case.normalize_length)
        assert not bool(torch.isnan(kl).any()) and not bool(torch.isnan(grad).any())
        if case.smoothing == 0.0 or not bool(case.mask.any()):
            continue
        x = case.logits.double()[None]
        want = C.label_smoothing_loss(x, case.target[None], case.mask[None, None], case.smoothing)  # (/ B = 1)
        assert abs(float(stats[0]) - float(want)) < 1e-9 * max(1.0, abs(float(want))), case.name
        if case.name != "ties":
            acc = C.th_accuracy(x, case.target[None], case.mask[None, None])
            assert abs(float(stats[1] / stats[2]) - float(acc)) < 1e-6, case.name
        # the gradient is the derivative of the KL sum
        xg = case.logits.double().clone().requires_grad_()
        C.label_smoothing_loss(xg[None], case.target[None], case.mask[None, None], case.smoothing).backward()
        denom = float(stats[2]) if case.normalize_length else 1.0
        assert float((xg.grad * case.grad_scale / denom - grad).abs().max()) < 1e-12, case.name


def test_label_smoothing_case_conditions():
    cases = {c.name: c for c in TC.lsm_cases()}
    assert {c.V for c in cases.values()} >= set(TC.LSM_V) and {c.rows for c in cases.values()} >= set(TC.LSM_ROWS)
    assert {c.smoothing for c in cases.values()} == set(TC.LSM_SMOOTHING) and {c.normalize_length for c in cases.values()} == {False, True}
    for V in TC.LSM_V:
        assert {c.ld for c in cases.values() if c.V == V} >= {V, TC.pad64(V)}
    ref = TC.LsmReference(cases["all_masked"])
    assert not bool(ref.stats.any()) and not bool(ref.grad.any())
    ties = cases["ties"]
    ref = TC.LsmReference(ties)
    top = ties.logits.max(1).values
    assert [int((ties.logits[r] == top[r]).sum()) for r in range(3)] == [2, 2, 2]
    hits = (ties.logits.argmax(1) == ties.target)[3:].sum()  # the rows without a tie
    assert float(ref.stats[1]) == 1.0 + float(hits)         # of the three tied rows only the one with the target at the FIRST maximum


def test_embedding_cases_are_exact_in_float32():
    for rows, L, D, V in TC.EMBED_FWD:
        for positive in (False, True):
            c = TC.embed_forward_case(rows, L, D, V, positive=positive)
            assert TC.embed_magnitude(c) < 2 ** 24
            assert int(c["tokens"].min()) < 0 or rows < 3
            assert int(c["tokens"].max()) >= V
            want = TC.embed_forward_expected(c)
            assert torch.equal(want.float().long(), want)
            if positive:
                assert int(want.min()) > 0
    g = torch.Generator().manual_seed(0)
    for pattern in TC.EMBED_PATTERNS:
        for rows in TC.EMBED_BWD_ROWS:
            c = TC.embed_backward_case(pattern, rows, 8)
            assert TC.embed_magnitude(c) < 2 ** 24
            for keep in (None, c["keep"]):
                want = TC.embed_backward_expected(c, keep)
                assert torch.equal(want.float().long(), want)
    tok, V = TC.embed_tokens("counts", 2500, g)
    assert [int((tok == 7 + 256 * k).sum()) for k in range(6)] == list(TC.EMBED_COUNTS)
    assert int((tok % 256 == 7).sum()) == sum(TC.EMBED_COUNTS)
    tok, V = TC.embed_tokens("mod256", 1025, g)
    assert len(set((tok % 256).tolist())) == 1 and len(set(tok.tolist())) == 4
    tok, V = TC.embed_tokens("out_of_range", 1025, g)
    assert int(tok.min()) < 0 and int(tok.max()) >= V


# ---- planted defects ----------------------------------------------------------------------------------------------------------------
def ctc_rejection(name, defect, arg=None, utt=None):
    """-> (worst margin of the float32 test, of the bf16 test, the old whole-tensor metric) for the model with `defect`."""
    case, ref = TC.ctc_cases()[name], TC.ctc_reference(name)
    nll, grad = TC.ctc_model_batch(case, defect, arg, utt)
    m32, m16 = (worst(TC.ctc_margins(case, ref, nll, grad, bf16=bf16)) for bf16 in (False, True))
    return m32, m16, TC.old_rel(grad, ref.grad)


def rejected_by_both(name, defect):
    m32, m16, _ = ctc_rejection(name, defect)
    return min(m32, m16)


def test_defect_skip_across_equal_labels():
    for name in ("ring", "chunk4", "chunk7", "feasibility", "uniform66"):
        assert rejected_by_both(name, "skip_equal") >= REJECT, name


# (case, state whose carry is dropped, the utterance it is dropped in, whether the old norm is blind to it)
CARRY = [("chunk4", 64, 6, True), ("chunk7", 64, 5, True), ("chunk7", 256, 6, True), ("chunk4", 128, 7, False)]


@pytest.mark.parametrize("name,state,utt,blind", CARRY)
def test_defect_dropped_carry_between_chunks(name, state, utt, blind):
    """Lane 0 of a chunk (a blank state) gets nothing from lane 63 of the chunk before, for ONE utterance.  What is lost are the
    alignments that pass through that blank: a few percent of the mass at a few frames where the neighbouring labels differ (the first
    three: the float32 per-row check rejects it, the whole-tensor bound of test_ctc_loss_grad passes it), the whole utterance where
    they are equal (the last: nothing is blind to that).  alpha, beta and the occupancies are the same code for both output types, so
    it is the float32 check - the tighter one - that the defect has to get past; the bf16 margin is printed."""
    m32, m16, rel = ctc_rejection(name, "drop_carry", state, utt)
    print("drop_carry %s state %d utt %d: float32 margin %.3g, bf16 margin %.3g, old rel %.3g" % (name, state, utt, m32, m16, rel))
    assert m32 >= REJECT
    assert (rel < TC.OLD_NORM_TOL) == blind


def test_defect_last_step_of_the_prefetch_ring():
    assert rejected_by_both("ring", "drop_last_step") >= REJECT
    # and it is the tlen % 4 == 1 utterances (tlen 5, 9, 9) that show it; tlen = 1 has no step to drop
    case, ref = TC.ctc_cases()["ring"], TC.ctc_reference("ring")
    nll, _ = TC.ctc_model_batch(case, "drop_last_step")
    off = ((nll - ref.nll).abs() > 1e-9).tolist()
    assert off == [False, False, False, False, True, False, False, False, True, True]


def repeated_label(case, utt):
    """A label of utterance `utt` that occurs more than once, never adjacent to itself, and is not the blank."""
    ys = case.labels(utt)
    for l in ys:
        at = [i for i, y in enumerate(ys) if y == l]
        if len(at) >= 2 and l != case.blank and all(b - a > 1 for a, b in zip(at[:-1], at[1:])):
            return l
    raise AssertionError("no repeated label")


@pytest.mark.parametrize("name,utt,blind", [("chunk7", 8, True), ("chunk4", 0, False), ("chunk7", 7, False)])
def test_defect_repeated_label_counted_once(name, utt, blind):
    """ONE label of ONE utterance loses the occupancy of its later occurrences.  Where the alignment is sharp that is a whole unit at
    one frame, which the old norm sees at these batch sizes; in the flat utterance of chunk7 (A B A over 236 frames) it is a few
    percent at many frames: rejected per row (float32 margin; the bf16 one is printed), passed by the whole-tensor bound."""
    case = TC.ctc_cases()[name]
    m32, m16, rel = ctc_rejection(name, "repeat_once", repeated_label(case, utt), utt)
    print("repeat_once %s utt %d: float32 margin %.3g, bf16 margin %.3g, old rel %.3g" % (name, utt, m32, m16, rel))
    assert m32 >= REJECT
    assert (rel < TC.OLD_NORM_TOL) == blind
    if not blind:
        assert m16 >= REJECT


def test_defect_blank_valued_label():
    for name in ("chunk4", "chunk7", "uniform66"):
        assert rejected_by_both(name, "blank_label") >= REJECT, name


def test_defect_rows_past_the_length_not_zeroed():
    for name in ("ring", "chunk4", "feasibility", "addr_unaligned"):
        assert rejected_by_both(name, "tail_rows") >= REJECT, name


def lsm_rejection(case, **defect):
    ref = TC.LsmReference(case)
    args = dict(logits=case.logits, target=case.target, mask=case.mask, smoothing=case.smoothing, grad_scale=case.grad_scale,
                normalize_length=case.normalize_length)
    args.update(defect)
    stats, _, grad = TC.lsm_float64(**args)
    return min(worst(TC.lsm_margins(case, ref, stats, grad, bf16=bf16)) for bf16 in (False, True))


def test_label_smoothing_model_passes_and_defects_fail():
    cases = TC.lsm_cases()
    for case in cases:
        assert lsm_rejection(case) <= 1e-3, case.name
    # 7: off = s / V instead of s / (V - 1): a relative change of 1 / V - the small vocabularies are there to catch it
    seen = {case.V: lsm_rejection(case, off_div=case.V) for case in cases if case.smoothing > 0 and bool(case.mask.any())}
    assert seen[2] >= REJECT and seen[7] >= REJECT, seen
    # 8: the argmax tie resolved to the last index
    ties = [c for c in cases if c.name == "ties"][0]
    assert lsm_rejection(ties, tie="last") == math.inf
    # 9: normalize_length dividing by the rows instead of the unmasked tokens
    seen = 0
    for case in cases:
        if case.normalize_length and 0 < int(case.mask.sum()) < case.rows:
            assert lsm_rejection(case, normalize_length=False, grad_scale=case.grad_scale / case.rows) >= REJECT, case.name
            seen += 1
    assert seen >= 3


def test_embedding_defects_break_equality():
    # 10: positional row r // L instead of r % L
    for rows, L, D, V in TC.EMBED_FWD[1:]:
        c = TC.embed_forward_case(rows, L, D, V)
        assert not torch.equal(TC.embed_forward_expected(c, defect="pos_div"), TC.embed_forward_expected(c))
    # 11: the rows of a second 1024-row stage dropped - every pattern, with and without row_keep, at 1025 rows and beyond
    for pattern in TC.EMBED_PATTERNS:
        for rows in (1025, 2500):
            c = TC.embed_backward_case(pattern, rows, 8)
            for keep in (None, c["keep"]):
                if rows == 1025 and keep is not None and float(keep[1024]) == 0:
                    continue
                if rows == 1025 and not bool(c["g"][1024].any()):
                    continue
                assert not torch.equal(TC.embed_backward_expected(c, keep, defect="second_stage"), TC.embed_backward_expected(c, keep)), \
                    (pattern, rows)
    # and 1023 / 1024 rows have no second stage
    c = TC.embed_backward_case("mod256", 1024, 8)
    assert torch.equal(TC.embed_backward_expected(c, defect="second_stage"), TC.embed_backward_expected(c))
