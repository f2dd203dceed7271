"""Inputs, float64 references and comparators of the token-loss tests (test_token_loss_cases_cpu.py, test_token_loss_gpu.py): the CTC
kernels of csrc/ctc.hip, the label-smoothing loss and the embedding kernels of csrc/decoder_kernels.hip.  Nothing here needs a device.

CTC has three references that share no code: ctc_float64 (torch's F.ctc_loss in float64 + autograd, zero_infinity as the kernels apply
it), ctc_counting (all-zero logits: exact Python-integer alignment counts, gradients as Fractions, no torch) and ctc_single_alignment
(the closed form of an utterance that has exactly ONE alignment).  ctc_model is a fourth, a log-space float64 model of what the kernels
do that can carry one planted defect: the CPU test uses it to show that every check of the GPU test rejects every defect.

The embedding cases hold small integers (table, positional rows, upstream gradient), xscale is a power of two and 1 / (1 - p) is 1 or
2: every product and every sum is exact in float32 in any order, with or without FMA contraction, and the device result must EQUAL an
int64 index_add_.

row_err is the comparator: per-row ||got_i - want_i||, never a whole-tensor norm.
"""
import math
from fractions import Fraction

import numpy as np
import torch

F32_EPS = 2.0 ** -24      # half an ulp of float32 at 1
BF16_ULP = 2.0 ** -8      # one bf16 ulp, relative
NLL_TOL = 1e-5            # |got - want| <= NLL_TOL * max(1, |want|), per utterance
GRAD_FACTOR = 4.0         # a kernel's row may err by 4 x what float32 torch errs by on the same case
OLD_NORM_TOL = 5e-3       # the whole-tensor bound of test_ctc_loss_grad, kept to show what it does not see


def pad64(n):
    return (n + 63) // 64 * 64


def row_err(got, want):
    """(..., rows, cols) -> (..., rows) float64: ||got_i - want_i|| of every row."""
    return (got.double() - want.double()).norm(dim=-1)


def old_rel(got, want):
    """The whole-tensor metric of test_ctc_loss_grad."""
    return float((got.double() - want.double()).norm() / (want.double().norm() + 1e-30))


# ---- CTC: references ----------------------------------------------------------------------------------------------------------------
def extended(ys, blank):
    ext = [blank]
    for y in ys:
        ext += [int(y), blank]
    return ext


def adjacent_repeats(ys):
    return sum(1 for a, b in zip(ys[:-1], ys[1:]) if a == b)


def ctc_float64(logits, ys, hlens, ylens, blank, grad_scale, dtype=torch.float64):
    """logits (B, T, V), ys (B, Lmax), hlens / ylens (B,) -> (nll (B,), grad (B, T, V)) in `dtype`: log-softmax + F.ctc_loss
    (reduction none) + autograd of grad_scale * sum of the finite losses.  zero_infinity as the kernels apply it: an utterance without
    an alignment has nll = inf and a zero gradient and adds nothing to the sum.  hlens are clamped to T; an utterance of no frames
    with labels is infeasible, without labels it costs nothing."""
    B, T, V = logits.shape
    hl = torch.as_tensor(hlens).long().clamp(max=T)
    yl = torch.as_tensor(ylens).long()
    x = logits.to(dtype).clone().requires_grad_()
    lp = torch.log_softmax(x, -1).transpose(0, 1)
    args = (lp, torch.as_tensor(ys).long(), hl.clamp(min=1), yl)
    with torch.no_grad():
        nll = torch.nn.functional.ctc_loss(*args, blank=blank, reduction="none", zero_infinity=False).clone()
    live = hl >= 1
    nll[~live] = torch.where(yl[~live] == 0, 0.0, math.inf).to(dtype)
    per = torch.nn.functional.ctc_loss(*args, blank=blank, reduction="none", zero_infinity=True)
    (per * live.to(dtype)).sum().mul(grad_scale).backward()
    grad = x.grad.clone()
    grad[torch.isinf(nll)] = 0.0
    return nll, grad


def _count_tables(ys, T, blank):
    ext = extended(ys, blank)
    S = len(ext)
    a = [[0] * S for _ in range(T)]
    b = [[0] * S for _ in range(T)]
    a[0][0] = 1
    if S > 1:
        a[0][1] = 1
    for t in range(1, T):
        for s in range(S):
            n = a[t - 1][s]
            if s >= 1:
                n += a[t - 1][s - 1]
            if s >= 2 and ext[s] != ext[s - 2]:
                n += a[t - 1][s - 2]
            a[t][s] = n
    b[T - 1][S - 1] = 1
    if S > 1:
        b[T - 1][S - 2] = 1
    for t in range(T - 2, -1, -1):
        for s in range(S):
            n = b[t + 1][s]
            if s + 1 < S:
                n += b[t + 1][s + 1]
            if s + 2 < S and ext[s + 2] != ext[s]:
                n += b[t + 1][s + 2]
            b[t][s] = n
    return ext, a, b


def count_alignments(ys, T, blank):
    """Number of length-T alignments of `ys` (exact)."""
    if T < 1:
        return 1 if len(ys) == 0 else 0
    ext, a, _ = _count_tables(list(ys), T, blank)
    return a[T - 1][-1] + (a[T - 1][-2] if len(ext) > 1 else 0)


def ctc_counting(ys, T, V, blank):
    """All-zero logits: every alignment has probability V^-T, so with N alignments (Python integers, forward table a, backward table
    b) nll = T log V - log N and grad[t, v] = 1 / V - sum_{s: ext[s] = v} a[t][s] b[t][s] / N, formed as Fractions.  The skip into
    state s is allowed iff ext[s] != ext[s - 2]: that one rule also covers a label that equals the blank.
    -> (N, nll, grad (T, V) float64 tensor); N == 0: (0, inf, zeros)."""
    ext, a, b = _count_tables(list(ys), T, blank)
    S = len(ext)
    N = a[T - 1][S - 1] + (a[T - 1][S - 2] if S > 1 else 0)
    grad = torch.zeros(T, V, dtype=torch.float64)
    if N == 0:
        return 0, math.inf, grad
    for t in range(T):
        num = [0] * V
        for s in range(S):
            num[ext[s]] += a[t][s] * b[t][s]
        for v in range(V):
            grad[t, v] = float(Fraction(1, V) - Fraction(num[v], N))
    return N, T * math.log(V) - math.log(N), grad


def single_alignment_path(ys, tlen, blank):
    """The one alignment of an utterance with tlen == U + adjacent repeats (a blank between equal neighbours, nowhere else), or of
    an empty target (all blank).  No label may equal the blank."""
    ys = [int(y) for y in ys]
    assert blank not in ys
    if not ys:
        return [blank] * tlen
    assert tlen == len(ys) + adjacent_repeats(ys)
    pi = [ys[0]]
    for prev, y in zip(ys[:-1], ys[1:]):
        if prev == y:
            pi.append(blank)
        pi.append(y)
    return pi


def ctc_single_alignment(logits, ys, tlen, blank, grad_scale):
    """logits (T, V) of one utterance -> (nll, grad (T, V)) float64: nll = -sum_t logp[t, pi_t], row t = softmax - onehot(pi_t)."""
    pi = single_alignment_path(ys, tlen, blank)
    lp = torch.log_softmax(logits.double(), -1)
    idx = torch.tensor(pi)
    nll = -float(lp[torch.arange(tlen), idx].sum())
    grad = torch.zeros_like(lp)
    grad[:tlen] = torch.exp(lp[:tlen])
    grad[torch.arange(tlen), idx] -= 1.0
    return nll, grad * grad_scale


CTC_DEFECTS = ("skip_equal", "drop_carry", "drop_last_step", "repeat_once", "blank_label", "tail_rows")


def ctc_model(logits, ys, tlen, blank, grad_scale, defect=None, arg=None):
    """Log-space float64 model of ctc_alpha_body / ctc_beta_body / ctc_dlogits_kernel for one utterance, logits (T, V) -> (nll, grad
    (T, V)), with at most one planted defect:
      skip_equal      the skip transition s - 2 -> s is allowed across equal labels too
      drop_carry      state `arg` (64, 128, 256: lane 0 of a chunk) of the alpha recursion gets nothing from the chunk before
      drop_last_step  the alpha step t = tlen - 1 is not taken when tlen % 4 == 1 (the prefetch ring's remainder)
      repeat_once     label `arg`: only its first occurrence's occupancy is subtracted
      blank_label     a label that equals the blank is not added to the blank's occupancy
      tail_rows       rows t >= tlen are not zeroed (they hold the softmax)"""
    assert defect is None or defect in CTC_DEFECTS
    T, V = logits.shape
    lp = torch.log_softmax(logits.double(), -1).numpy()
    ext = np.array(extended(ys, blank))
    S = len(ext)
    grad = np.zeros((T, V))
    if defect == "tail_rows":
        grad[tlen:] = np.exp(lp[tlen:])
    ninf = -np.inf
    s_idx = np.arange(S)
    skip = np.zeros(S, bool)
    skip[2:] = ext[2:] != ext[:-2]
    if defect == "skip_equal":
        skip[2:] = (s_idx[2:] & 1) == 1
    if tlen < 1:
        return (0.0 if S == 1 else math.inf), torch.from_numpy(grad) * grad_scale

    def lae3(x0, x1, x2):
        with np.errstate(invalid="ignore"):
            return np.logaddexp(np.logaddexp(x0, x1), x2)

    alpha = np.full((tlen, S), ninf)
    alpha[0, 0] = lp[0, blank]
    if S > 1:
        alpha[0, 1] = lp[0, ext[1]]
    for t in range(1, tlen):
        if defect == "drop_last_step" and tlen % 4 == 1 and t == tlen - 1:
            alpha[t] = alpha[t - 1]
            continue
        a0 = alpha[t - 1]
        a1 = np.concatenate([[ninf], a0])[:S]
        a2 = np.where(skip, np.concatenate([[ninf, ninf], a0])[:S], ninf)
        if defect == "drop_carry" and arg < S:
            a1[arg] = ninf
            a2[arg] = ninf
        alpha[t] = lae3(a0, a1, a2) + lp[t, ext]
    beta = np.full((tlen, S), ninf)  # with the step's emission
    beta[tlen - 1, S - 1] = lp[tlen - 1, ext[S - 1]]
    if S > 1:
        beta[tlen - 1, S - 2] = lp[tlen - 1, ext[S - 2]]
    skipb = np.zeros(S, bool)
    skipb[:-2] = ext[2:] != ext[:-2]
    if defect == "skip_equal":
        skipb[:-2] = (s_idx[:-2] & 1) == 1
    for t in range(tlen - 2, -1, -1):
        b0 = beta[t + 1]
        b1 = np.concatenate([b0, [ninf]])[1:]
        b2 = np.where(skipb, np.concatenate([b0, [ninf, ninf]])[2:], ninf)
        beta[t] = lae3(b0, b1, b2) + lp[t, ext]
    fin = alpha[tlen - 1, S - 1]
    if S > 1:
        fin = np.logaddexp(fin, alpha[tlen - 1, S - 2])
    if fin == ninf:
        return math.inf, torch.from_numpy(grad) * grad_scale
    nll = -float(fin)
    with np.errstate(invalid="ignore"):
        w = np.exp(alpha + beta - lp[:tlen][:, ext] + nll)  # (tlen, S) state occupancies
    w = np.nan_to_num(w, nan=0.0)
    counted = np.ones(S, bool)
    if defect == "repeat_once":
        at = np.nonzero((ext == arg) & (s_idx & 1 == 1))[0]
        counted[at[1:]] = False
    if defect == "blank_label":
        counted[(ext == blank) & (s_idx & 1 == 1)] = False
    occ = np.zeros((tlen, V))
    for s in range(S):
        if counted[s]:
            occ[:, ext[s]] += w[:, s]
    grad[:tlen] = np.exp(lp[:tlen]) - occ
    return nll, torch.from_numpy(grad) * grad_scale


# ---- CTC: cases ---------------------------------------------------------------------------------------------------------------------
class CtcCase:
    """logits (B, T, V) float32, ys (B, Lmax) int64 (zero-padded past ylens), hlens / ylens lists.  ld: the row stride the device
    buffer gets, offset: floats the device view starts into its buffer (1: the base is not 16-byte aligned).  single: utterances that
    have exactly one alignment, infeasible: those that have none; uniform: all-zero logits (ctc_counting is the reference)."""

    def __init__(self, name, logits, ys, hlens, ylens, blank, ld, grad_scale=1.0, offset=0, single=(), infeasible=(), uniform=False):
        self.name, self.logits, self.ys, self.hlens, self.ylens, self.blank = name, logits, ys, list(hlens), list(ylens), blank
        self.B, self.T, self.V = logits.shape
        self.ld, self.grad_scale, self.offset, self.uniform = ld, grad_scale, offset, uniform
        self.single, self.infeasible = tuple(single), tuple(infeasible)
        self.Lmax = ys.shape[1]
        assert ld >= self.V and self.Lmax >= 1 and max(self.ylens) <= self.Lmax
        assert int(ys.min()) >= 0 and int(ys.max()) < self.V and 0 <= blank < self.V  # nothing a kernel would read out of bounds with

    def tlen(self, b):
        return min(self.hlens[b], self.T)

    def labels(self, b):
        return [int(y) for y in self.ys[b, :self.ylens[b]]]

    def device_logits(self, device, pad_value=50.0):
        """(B * T, V) view with row stride ld, `offset` floats into its buffer; the pad columns [V, ld) hold `pad_value` (a kernel
        that read them would show it: the largest logit is far below)."""
        rows = self.B * self.T
        buf = torch.full((rows * self.ld + 4,), pad_value, dtype=torch.float32)
        view = buf[self.offset:self.offset + rows * self.ld].view(rows, self.ld)
        view[:, :self.V] = self.logits.reshape(rows, self.V)
        buf = buf.to(device)
        return buf[self.offset:self.offset + rows * self.ld].view(rows, self.ld)[:, :self.V]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _labels(g, n, V, blank, repeats=0):
    """n random labels != blank, with exactly `repeats` more adjacent equal pairs forced in at spread positions."""
    y = torch.randint(0, V - 1, (n,), generator=g)
    y = y + (y >= blank).long()
    for k in range(repeats):
        p = 1 + (k * 7919) % (n - 1)
        y[p] = y[p - 1]
    return y


def _pack(rows, Lmax):
    ys = torch.zeros(len(rows), Lmax, dtype=torch.long)
    for b, y in enumerate(rows):
        ys[b, :len(y)] = torch.as_tensor(y)
    return ys


def ctc_ring_case():
    """The 4-step emission prefetch ring: tlen 1 .. 9 (every tlen % 4, the ring empty, partly and fully used) and hlens > T."""
    T, V, B, blank = 9, 11, 10, 0
    hlens = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12]
    ylens = [1, 1, 2, 0, 2, 3, 1, 4, 3, 2]
    g = _gen(11)
    rows = []
    for b in range(B):
        y = _labels(g, ylens[b], V, blank)
        if ylens[b] >= 2 and min(hlens[b], T) >= ylens[b] + adjacent_repeats(y.tolist()) + 1 and adjacent_repeats(y.tolist()) == 0:
            y[1] = y[0]
        rows.append(y)
    logits = torch.randn(B, T, V, generator=g) * 1.5
    return CtcCase("ring", logits, _pack(rows, 4), hlens, ylens, blank, 64, grad_scale=0.5)


def _chunk_case(name, seed, ylens, slack, T, V, blank, Lmax, abab_at, blank_label_at, flat_at=None):
    g = _gen(seed)
    rows, hlens, single = [], [], []
    for b, (U, sl) in enumerate(zip(ylens, slack)):
        y = _labels(g, U, V, blank)
        if b == abab_at:
            y = torch.tensor([(1 + blank) % V if i % 2 == 0 else (2 + blank) % V for i in range(U)])
        if b == blank_label_at:
            y[U // 3] = blank
            y[2 * U // 3] = blank
        if b == flat_at:
            y = torch.tensor([(1 + blank) % V, (2 + blank) % V, (1 + blank) % V])
            sl = T - U
        r = adjacent_repeats(y.tolist())
        rows.append(y)
        hlens.append(U + r + sl)
        if sl == 0 and b != blank_label_at:
            single.append(b)
    assert max(hlens) <= T
    logits = torch.randn(len(ylens), T, V, generator=g) * 1.5
    if flat_at is not None:
        logits[flat_at] *= 0.2
    logits[:, :, blank] += 2.0  # (the blank is the likeliest symbol, as in a trained model: the blank states carry mass)
    return CtcCase(name, logits, _pack(rows, Lmax), hlens, ylens, blank, pad64(V), grad_scale=2.0, single=single)


def ctc_chunk4_case():
    """The 4-chunk kernels on both sides of states 63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193 and at the last state 254: tlen
    from the single alignment (no slack) to five spare frames; labels from 39 symbols (non-adjacent repeats in every utterance),
    utterance 3 is ABAB..., utterance 5 holds the blank's value as a label twice."""
    return _chunk_case("chunk4", 21, [31, 32, 33, 63, 64, 65, 95, 96, 127, 2], [0, 1, 2, 5, 0, 1, 2, 5, 0, 3], 140, 40, 0, 127, 3, 5)


def ctc_chunk7_case():
    """The 7-chunk kernels (Lmax = 223: 447 states), a blank other than 0."""
    return _chunk_case("chunk7", 22, [128, 159, 160, 161, 191, 192, 193, 223, 3], [1, 2, 5, 0, 1, 2, 5, 0, 3], 236, 40, 39, 223, 2, 4, flat_at=8)


FEASIBILITY_PAIRS = [(1, 0), (2, 0), (2, 1), (32, 0), (32, 1), (32, 3), (64, 0), (64, 1), (64, 3)]  # (U, adjacent repeats)


def ctc_feasibility_case():
    """Every target twice: with tlen = U + repeats (one alignment) and with one frame fewer (none: inf, zero gradient)."""
    T, V, blank, Lmax = 67, 13, 0, 64
    g = _gen(31)
    rows, hlens, ylens, single, infeasible = [], [], [], [], []
    for U, r in FEASIBILITY_PAIRS:
        y = _labels(g, U, V, blank)
        for k in range(1, U):  # no repeat by chance, then exactly r of them
            while y[k] == y[k - 1]:
                y[k] = 1 + (int(y[k]) % (V - 1))
        for k in range(r):
            p = 1 + k * ((U - 1) // r) if U > 2 else 1
            y[p] = y[p - 1]
            if p + 1 < U and y[p + 1] == y[p]:
                y[p + 1] = 1 + (int(y[p + 1]) % (V - 1))
        assert adjacent_repeats(y.tolist()) == r, (U, r, y.tolist())
        for tl in (U + r, U + r - 1):
            (single if tl == U + r else infeasible).append(len(rows))
            rows.append(y)
            hlens.append(tl)
            ylens.append(U)
    logits = torch.randn(len(rows), T, V, generator=g) * 1.5
    return CtcCase("feasibility", logits, _pack(rows, Lmax), hlens, ylens, blank, 16, single=single, infeasible=infeasible)


def _cyclic(U, V, blank, repeats, blank_at=None):
    """Labels 1, 2, .., V - 1, 1, .. (blank 0 assumed): no adjacent repeat, every label many times; then `repeats` adjacent pairs."""
    assert blank == 0 and V >= 4
    y = [1 + i % (V - 1) for i in range(U)]
    for k in range(repeats):
        p = 2 + k * ((U - 3) // max(repeats, 1))
        y[p] = y[p - 1]
    if blank_at is not None:
        y[blank_at] = blank
    return y


def ctc_uniform_cases():
    """All-zero logits, (U, T) in (0, 5), (1, 1), (5, 9), (66, 78) - ten adjacent repeats and a label that equals the blank - and
    (223, 229): ctc_counting is the reference."""
    V, blank = 7, 0
    small = [([], 5), ([3], 1), ([1, 1, 2, 3, 1], 9), (_cyclic(66, V, blank, 10, blank_at=20), 78)]
    big = [(_cyclic(223, V, blank, 4), 229)]
    out = []
    for name, utts, T, Lmax in (("uniform66", small, 78, 66), ("uniform223", big, 229, 223)):
        ys = _pack([u[0] for u in utts], Lmax)
        out.append(CtcCase(name, torch.zeros(len(utts), T, V), ys, [u[1] for u in utts], [len(u[0]) for u in utts], blank, 8,
                           uniform=True))
    return out


ADDRESSING = [(11, 13), (11, 11), (97, 128), (4233, 4288), (5121, 5124)]  # (V, ld): ld % 4 != 0, ld == V, the float4 forms, V > 5120


def ctc_addressing_cases():
    """The scalar fallbacks of ctc_lse_kernel and ctc_dlogits_kernel against their float4 forms, each with blank 0, 3 and V - 1, and
    one view that starts one float into its buffer."""
    out = []
    for i, (V, ld) in enumerate(ADDRESSING):
        for blank in (0, 3, V - 1):
            g = _gen(400 + 10 * i + min(blank, 9))
            B, T = 2, 7
            rows = [_labels(g, 3, V, blank, repeats=1), _labels(g, 2, V, blank)]
            logits = torch.randn(B, T, V, generator=g) * 1.5
            out.append(CtcCase("addr_V%d_ld%d_blank%d" % (V, ld, blank), logits, _pack(rows, 3), [7, 9], [3, 2], blank, ld))
    g = _gen(499)
    rows = [_labels(g, 3, 97, 3, repeats=1), _labels(g, 2, 97, 3)]
    out.append(CtcCase("addr_unaligned", torch.randn(2, 7, 97, generator=g) * 1.5, _pack(rows, 3), [7, 5], [3, 2], 3, 128, offset=1))
    return out


_CTC = {}


def ctc_cases():
    if not _CTC:
        for c in [ctc_ring_case(), ctc_chunk4_case(), ctc_chunk7_case(), ctc_feasibility_case()] + ctc_uniform_cases() \
                + ctc_addressing_cases():
            _CTC[c.name] = c
    return _CTC


class CtcReference:
    """nll (B,) and grad (B, T, V) float64 (grad_scale folded in) of a case, and what the float32 checks allow:
    yard (B,): the worst row error of float32 CPU torch (F.ctc_loss + autograd) against that float64 reference, per utterance;
    floor (B,): 8 * 2^-24 * max(1, nll_b) * grad_scale - an occupancy is exp(alpha + beta + nll), and three float32 quantities of
    magnitude nll carry that much rounding into the exponent;  bound (B,) = max(4 * yard, floor): what a float32 gradient row of
    utterance b may be off by.  A bf16 row may be off by 2^-8 * ||want_row|| more (one bf16 ulp per element)."""

    def __init__(self, case):
        c = case
        if c.uniform:
            nll, grad = [], []
            for b in range(c.B):
                tl = c.tlen(b)
                _, n, gr = ctc_counting(c.labels(b), tl, c.V, c.blank)
                full = torch.zeros(c.T, c.V, dtype=torch.float64)
                full[:tl] = gr
                nll.append(n)
                grad.append(full * c.grad_scale)
            self.nll, self.grad = torch.tensor(nll, dtype=torch.float64), torch.stack(grad)
        else:
            self.nll, self.grad = ctc_float64(c.logits, c.ys, c.hlens, c.ylens, c.blank, c.grad_scale)
        nll32, grad32 = ctc_float64(c.logits, c.ys, c.hlens, c.ylens, c.blank, c.grad_scale, dtype=torch.float32)
        self.yard = row_err(grad32, self.grad).max(dim=1).values
        finite = torch.where(torch.isinf(self.nll), torch.zeros_like(self.nll), self.nll)
        self.floor = 8 * F32_EPS * finite.abs().clamp_min(1.0) * c.grad_scale
        self.bound = torch.maximum(GRAD_FACTOR * self.yard, self.floor)
        self.yard_nll = float(((nll32.double() - self.nll).abs()[~torch.isinf(self.nll)] / finite.abs().clamp_min(1.0)[~torch.isinf(self.nll)])
                              .max()) if bool((~torch.isinf(self.nll)).any()) else 0.0


_CTC_REF = {}


def ctc_reference(name):
    if name not in _CTC_REF:
        _CTC_REF[name] = CtcReference(ctc_cases()[name])
    return _CTC_REF[name]


def ctc_margins(case, ref, nll, grad, bf16=False):
    """What the GPU test asserts, as ratios error / allowed (a check passes at <= 1):
      nll    per utterance |got - want| / (1e-5 max(1, |want|)); inf where one is infinite and the other is not
      row    per row ||got - want|| / bound_b (+ 2^-8 ||want_row|| for bf16)
      exact  inf if a row t >= tlen, or a row of an utterance without an alignment, is not exactly zero
    nll (B,), grad (B, T, >= V): only the first V columns are compared here."""
    nll, grad = nll.double().cpu(), grad.double().cpu()[..., :case.V]
    inf_w, inf_g = torch.isinf(ref.nll), torch.isinf(nll)
    fin = ~inf_w & ~inf_g
    m_nll = math.inf if bool((inf_w != inf_g).any()) or bool(torch.isnan(nll).any()) else 0.0
    if bool(fin.any()):
        m_nll = max(m_nll, float(((nll - ref.nll).abs()[fin] / (NLL_TOL * ref.nll.abs().clamp_min(1.0)[fin])).max()))
    allowed = ref.bound[:, None].expand(case.B, case.T)
    if bf16:
        allowed = allowed + BF16_ULP * ref.grad.norm(dim=-1)
    err = row_err(grad, ref.grad)
    m_row = float((err / allowed).max()) if not bool(torch.isnan(err).any()) else math.inf
    exact = 0.0
    for b in range(case.B):
        if bool((grad[b, case.tlen(b):] != 0).any()) or (bool(inf_w[b]) and bool((grad[b] != 0).any())):
            exact = math.inf
    return {"nll": m_nll, "row": m_row, "exact": exact}


def ctc_model_batch(case, defect=None, arg=None, utt=None):
    """ctc_model on every utterance of a case -> (nll (B,), grad (B, T, V)); the defect is planted in utterance `utt` (None: in all)."""
    nll, grad = [], []
    for b in range(case.B):
        d = defect if utt is None or utt == b else None
        n, gr = ctc_model(case.logits[b], case.labels(b), case.tlen(b), case.blank, case.grad_scale, d, arg)
        nll.append(n)
        grad.append(gr)
    return torch.tensor(nll, dtype=torch.float64), torch.stack(grad)


# ---- label smoothing ----------------------------------------------------------------------------------------------------------------
def lsm_float64(logits, target, mask, smoothing, grad_scale, normalize_length, dtype=torch.float64, tie="first", off_div=None):
    """logits (rows, V), target (rows,) (-1 on masked rows: clamped to 0 as the reference model multiplies it by the mask), mask
    (rows,) 0 / 1 -> (stats (3,) = [sum of KL, correct, tokens], kl per row, grad (rows, V)) in `dtype`.
    KL(q || softmax) with q = 1 - smoothing at the target and smoothing / (V - 1) elsewhere, through xlogy (smoothing = 0: no NaN);
    correct counts argmax == target with ties resolved to the FIRST index; grad = grad_scale / denom * (softmax - q), denom = the
    number of unmasked tokens if normalize_length else 1; masked rows are zero.
    tie / off_div: the planted defects of the CPU test (`last`; smoothing divided by V instead of V - 1)."""
    rows, V = logits.shape
    x = logits.to(dtype)
    live = torch.as_tensor(mask) != 0
    tg = torch.as_tensor(target).long().clamp(min=0)
    off = smoothing / (V - 1 if off_div is None else off_div)
    q = torch.full_like(x, off)
    q.scatter_(1, tg[:, None], 1.0 - smoothing)
    logp = torch.log_softmax(x, -1)
    kl = (torch.xlogy(q, q) - q * logp).sum(1) * live.to(dtype)
    xn = x.numpy()
    am = np.argmax(xn, 1) if tie == "first" else V - 1 - np.argmax(xn[:, ::-1], 1)  # (numpy: the first occurrence, documented)
    correct = (torch.from_numpy(am) == tg) & live
    tokens = int(live.sum())
    denom = tokens if normalize_length else 1
    grad = (torch.exp(logp) - q) * live.to(dtype)[:, None] * (grad_scale / denom if denom else 0.0)
    stats = torch.stack([kl.sum(), correct.sum().to(dtype), torch.tensor(float(tokens), dtype=dtype)])
    return stats, kl, grad


class LsmCase:
    def __init__(self, name, logits, target, mask, smoothing, normalize_length, ld, grad_scale=0.5):
        self.name, self.logits, self.target, self.mask, self.smoothing = name, logits, target, mask, smoothing
        self.normalize_length, self.ld, self.grad_scale = normalize_length, ld, grad_scale
        self.rows, self.V = logits.shape
        live = mask != 0
        assert int(target[live].min() if bool(live.any()) else 0) >= 0 and int(target.max()) < self.V and ld >= self.V

    def device_logits(self, device, pad_value=90.0):
        buf = torch.full((self.rows, self.ld), pad_value, dtype=torch.float32)
        buf[:, :self.V] = self.logits
        return buf.to(device)[:, :self.V]


LSM_V = (2, 7, 255, 256, 257, 1000, 4233)
LSM_ROWS = (1, 5, 63, 64, 65, 130)
LSM_SMOOTHING = (0.0, 0.1, 0.5)


def _lsm_inputs(g, rows, V, masked="third"):
    logits = torch.randn(rows, V, generator=g) * 2.0
    target = torch.randint(0, V, (rows,), generator=g)
    # (a target that IS the argmax on half of the rows: the correct count is not trivially ~0)
    hit = torch.rand(rows, generator=g) < 0.5
    target = torch.where(hit, logits.argmax(1), target)
    mask = torch.ones(rows)
    if masked == "third":
        mask[torch.rand(rows, generator=g) < 1.0 / 3.0] = 0.0
        if rows == 1:
            mask[:] = 1.0
    elif masked == "all":
        mask[:] = 0.0
    target = torch.where(mask == 0, torch.full_like(target, -1), target)
    return logits, target, mask


def lsm_cases():
    out, k = [], 0
    for V in LSM_V:
        for ld in sorted({V, pad64(V)}):
            rows, s, nl = LSM_ROWS[k % 6], LSM_SMOOTHING[k % 3], (k // 3) % 2 == 1
            logits, target, mask = _lsm_inputs(_gen(700 + k), rows, V)
            out.append(LsmCase("V%d_ld%d_rows%d_s%g_%s" % (V, ld, rows, s, "len" if nl else "batch"), logits, target, mask, s, nl, ld))
            k += 1
    logits, target, mask = _lsm_inputs(_gen(790), 65, 257, masked="all")
    out.append(LsmCase("all_masked", logits, target, mask, 0.1, True, 320))
    # ties: the maximum at two columns - in two waves (5, 200) and in one thread's stride (0, 256)
    logits, target, mask = _lsm_inputs(_gen(791), 5, 257, masked="none")
    top = float(logits.max()) + 1.0
    for r, (c0, c1, tg) in enumerate([(5, 200, 200), (0, 256, 256), (5, 200, 5)]):
        logits[r, c0] = logits[r, c1] = top
        target[r] = tg
    out.append(LsmCase("ties", logits, target, mask, 0.1, False, 320))
    logits, target, mask = _lsm_inputs(_gen(792), 5, 4233)
    out.append(LsmCase("shift40", logits + 40.0, target, mask, 0.1, True, 4288))
    return out


class LsmReference:
    """stats / kl / grad in float64, and what float32 CPU torch does with the same formulas: yard (worst row error of its gradient),
    yard_kl (error of its KL sum).  A gradient row may be off by bound = max(4 * yard, floor), floor = 8 * 2^-24 * max(1, max |x|)
    * grad_scale / denom: softmax = exp(x - lse), and x, lse and their difference are float32 of magnitude max |x| - the same
    reasoning as for the CTC occupancies."""

    def __init__(self, case):
        c = case
        args = (c.logits, c.target, c.mask, c.smoothing, c.grad_scale, c.normalize_length)
        self.stats, self.kl, self.grad = lsm_float64(*args)
        s32, _, g32 = lsm_float64(*args, dtype=torch.float32)
        self.yard = float(row_err(g32, self.grad).max())
        self.yard_kl = abs(float(s32[0]) - float(self.stats[0]))
        tokens = float(self.stats[2])
        self.gscale = c.grad_scale / (tokens if c.normalize_length else 1.0) if tokens else 0.0
        self.floor = 8 * F32_EPS * max(1.0, float(c.logits.abs().max())) * self.gscale
        self.bound = max(GRAD_FACTOR * self.yard, self.floor)
        self.kl_tol = c.rows * 2.0 ** -20 * max(1.0, abs(float(self.stats[0])))


def lsm_margins(case, ref, stats, grad, bf16=False):
    """Ratios error / allowed of the GPU test's checks: kl (the KL sum), row (gradient rows), exact (inf unless the correct and token
    counts are the exact integers and masked rows exactly zero), rowsum (float32 only: each row sums to zero within V 2^-24 scale)."""
    stats, grad = stats.double().cpu(), grad.double().cpu()[:, :case.V]
    exact = 0.0 if float(stats[1]) == float(ref.stats[1]) and float(stats[2]) == float(ref.stats[2]) else math.inf
    if bool((grad[case.mask == 0] != 0).any()) or bool(torch.isnan(grad).any()) or bool(torch.isnan(stats).any()):
        exact = math.inf
    allowed = torch.full((case.rows,), ref.bound, dtype=torch.float64)
    if bf16:
        allowed = allowed + BF16_ULP * ref.grad.norm(dim=-1)
    live = case.mask != 0
    m_row = float((row_err(grad, ref.grad) / allowed)[live].max()) if ref.bound > 0 and bool(live.any()) else 0.0
    out = {"kl": abs(float(stats[0]) - float(ref.stats[0])) / ref.kl_tol, "row": m_row, "exact": exact}
    if not bf16 and ref.gscale > 0:
        out["rowsum"] = float(grad.sum(1).abs().max()) / (case.V * F32_EPS * ref.gscale)
    return out


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
EMBED_FWD = [(1, 1, 64, 5), (7, 7, 256, 97), (33, 11, 257, 300), (1240, 31, 512, 4233), (65, 13, 1024, 1000)]  # (rows, L, D, V)
EMBED_BWD_D = (1, 64, 256, 257, 512, 1024)
EMBED_BWD_ROWS = (1, 8, 9, 1023, 1024, 1025, 2500)
EMBED_PATTERNS = ("one_id", "mod256", "interleaved", "counts", "v3", "out_of_range")
EMBED_COUNTS = (1, 7, 8, 9, 16, 17)


def clamp_tokens(tok, V):
    return tok.long().clamp(0, V - 1)


def embed_tokens(pattern, rows, g):
    """-> (tokens (rows,) int32, V).  Workgroup t % 256 owns token t: `mod256` and `interleaved` give one workgroup every row (the
    second as a, b, a, b: every run in registers is one row long); `counts` gives one workgroup ids that occur exactly 1, 7, 8, 9, 16
    and 17 times, once as runs and once scattered among other rows (the 8-row walk and its clamped duplicates)."""
    if pattern == "one_id":
        return torch.full((rows,), 5, dtype=torch.int32), 1000
    if pattern == "mod256":
        ids = torch.tensor([3, 259, 515, 771])
        return ids[torch.randint(0, 4, (rows,), generator=g)].int(), 1000
    if pattern == "interleaved":
        return torch.tensor([3, 259])[torch.arange(rows) % 2].int(), 1000
    if pattern == "counts":
        V = 1600
        runs = torch.cat([torch.full((n,), 7 + 256 * k) for k, n in enumerate(EMBED_COUNTS)])
        if rows < runs.numel():
            return runs[:rows].int(), V
        rest = torch.randint(0, V, (rows - runs.numel(),), generator=g)
        rest = rest + (rest % 256 == 7).long()  # (no further occurrence of the counted ids)
        tok = torch.cat([runs, rest])
        if rows % 2 == 0:  # scattered: the counted rows keep their order but other workgroups' rows lie between them
            tok = tok[torch.randperm(rows, generator=g)]
        return tok.int(), V
    if pattern == "v3":
        return torch.randint(0, 3, (rows,), generator=g).int(), 3
    if pattern == "out_of_range":
        return torch.randint(-3, 97 + 4, (rows,), generator=g).int(), 97
    raise ValueError(pattern)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g)


def embed_forward_case(rows, L, D, V, positive=False, seed=0):
    """-> dict(tokens int32 (with -1 and V + 3 among them), table (V, D), pe (L, D) int64, xscale).  positive: table and pe >= 1 (the
    p = 0.5 test reads the dropout mask off out != 0)."""
    g = _gen(900 + seed + rows + D)
    tok = torch.randint(0, V, (rows,), generator=g)
    if rows >= 3:
        tok[rows // 3] = -1
        tok[2 * rows // 3] = V + 3
    elif V > 1:
        tok[0] = V + 3
    table = _ints(g, (V, D), 1, 8) if positive else _ints(g, (V, D), -8, 8)
    pe = _ints(g, (L, D), 1, 4) if positive else _ints(g, (L, D), -4, 4)
    return dict(rows=rows, L=L, D=D, V=V, tokens=tok.int(), table=table, pe=pe, xscale=4.0)


def embed_forward_expected(c, defect=None):
    """int64 (rows, D): table[clamp(tok)] * xscale + pe[r % L].  defect `pos_div`: pe[r // L]."""
    r = torch.arange(c["rows"])
    pos = (r // c["L"]).clamp(max=c["L"] - 1) if defect == "pos_div" else r % c["L"]
    return c["table"][clamp_tokens(c["tokens"], c["V"])] * int(c["xscale"]) + c["pe"][pos]


def embed_backward_case(pattern, rows, D, seed=0):
    g = _gen(1000 + seed + 7 * rows + D + 31 * EMBED_PATTERNS.index(pattern))
    tok, V = embed_tokens(pattern, rows, g)
    keep = (torch.rand(rows, generator=g) < 2.0 / 3.0).float()
    return dict(pattern=pattern, rows=rows, D=D, V=V, tokens=tok, g=_ints(g, (rows, D), -8, 8), dtable0=_ints(g, (V, D), -16, 16),
                keep=keep, xscale=16.0)


def embed_backward_expected(c, row_keep=None, factor=None, defect=None):
    """int64 (V, D): dtable0 + index_add of g * xscale (* factor (rows, D): the dropout's 0 / 2) over the kept rows.
    defect `second_stage`: the rows from 1024 on are lost."""
    contrib = c["g"] * int(c["xscale"])
    if factor is not None:
        contrib = contrib * factor
    sel = torch.ones(c["rows"], dtype=torch.bool) if row_keep is None else row_keep != 0
    if defect == "second_stage":
        sel = sel & (torch.arange(c["rows"]) < 1024)
    out = c["dtable0"].clone()
    out.index_add_(0, clamp_tokens(c["tokens"], c["V"])[sel], contrib[sel])
    return out


def embed_magnitude(c):
    """Largest |value| any partial sum of the case can reach."""
    if "g" in c:
        return int(c["dtable0"].abs().max()) + c["rows"] * int(c["g"].abs().max()) * int(c["xscale"]) * 2
    return (int(c["table"].abs().max()) * int(c["xscale"]) + int(c["pe"].abs().max())) * 2
