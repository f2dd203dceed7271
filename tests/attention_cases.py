"""Inputs, references and comparators of the attention tests (test_attention_cases_cpu.py, test_attention_exact_gpu.py and the
per-row gradient tests of test_train_kernels_gpu.py).  Nothing here needs a device.

selector_case() builds inputs whose softmax rows are one-hot BY CONSTRUCTION: key j of head h carries a random +-amplitude sign code
in its 64 features, query i carries the code of key target(i), so score(i, target) = 64 amplitude^2 * scale and every other score is
a random walk far below it.  All values are exact in bf16 and all products and sums exact in float32, V lies in [1, 2), and the
builder asserts - from a float64 softmax of what it built - that every row's off-target mass is <= 2^-14.  The output error is then
<= 2 * 2 * 2^-14 = 2^-12, a sixteenth of half a bf16 ulp in [1, 2): a bf16 context row must EQUAL the selected V row bit for bit, and
which key, which head, which batch, which mask cell a kernel used is pinned without a tolerance.

rowwise_err() is the per-row comparator of the gradient tests; relpos_float64 / decoder_float64 are the float64 autograd references
and rounded_reference_relpos / rounded_reference_decoder float64 models of the backward kernels that round where the kernels round
(attention_bwd.hip, decoder_kernels.hip): the error of the model against float64 autograd is the yardstick the kernels are held to.
"""
import math

import numpy as np
import torch

DK = 64
MASKED = -10000.0
OFF_MASS = 2.0 ** -14   # per-row off-target probability mass a selector case may have
CTX_TOL = 2.0 ** -12    # = 2 (|V| < 2) * 2 (mass moved off and on) * OFF_MASS: what a float32 context may differ by
PROB_TOL = 2.0 ** -13
PERMS = ("identity", "reversal", "stride")
CARRIERS = ("k", "pos", "k+bias")
FLIPS = 4               # signs in which a secondary key differs from its primary


def bf16_round(x):
    """float64 -> the nearest bf16 value (through float32, as the kernels' conversions go), as float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32_round(x):
    return x.to(torch.float32).to(torch.float64)


def relpos_lens(b, T):
    return [T, max(1, T - 37), 1][:b]


# ---- selector inputs ----------------------------------------------------------------------------------------------------------------
def permutation(name, n, count):
    """Targets of queries 0 .. count-1 among n items (queries past n wrap around)."""
    i = np.arange(count)
    if name == "identity":
        return i % n
    if name == "reversal":  # early queries pick the LAST tile: the running max is replaced in every tile, alpha rescales a non-empty sum
        return n - 1 - i % n
    if name == "stride":    # neighbours land in different 16- and 64-key tiles
        s = 37
        while math.gcd(s, n) != 1:
            s += 1
        return (i * s + 5) % n
    raise ValueError(name)


class SelectorCase:
    """q (B, Tq, H, 64), k / val (Bk, Tk, H, 64), pos (Tk, H, 64), u / v (H, 64): float64 tensors of bf16-exact values.
    pri / sec (B, Tq): the key each query selects, and the one it selects when its primary is masked (-1: it has none)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def dm(self):
        return self.heads * DK

    def qkv(self):
        """(B * T, 3 * dm) bf16: rows [q | k | v] of the encoder's attention (Tq == Tk, no key groups)."""
        assert self.T_q == self.T_k and self.kv_group == 1
        rows = self.b * self.T_q
        return torch.cat([self.q.reshape(rows, -1), self.k.reshape(rows, -1), self.val.reshape(rows, -1)], 1).to(torch.bfloat16)

    def rows(self, name):
        x = getattr(self, name)
        return x.reshape(-1, self.dm).to(torch.bfloat16)

    def flagged(self):
        """(B, Tq) bool: the queries whose primary the per-(query, key) mask hides - two of every three, so that inside every 16-row
        tile some rows see their primary and some do not."""
        i = torch.arange(self.T_q)[None, :] + torch.arange(self.b)[:, None]
        return (i % 3 != 1) & (self.sec >= 0)

    def variants(self):
        return ("pad", "pad_sec", "cell") if self.secondary else ("nomask", "pad", "cell")

    def mask(self, variant):
        """None, the (Bk, Tk) padding mask (`pad_sec`: with every primary that has a secondary hidden too) or the (B, Tq, Tk) mask
        with the padding folded in (`cell` with secondaries: the single cell (i, pri(i)) of the flagged queries hidden as well)."""
        if variant == "nomask":
            return None
        j = torch.arange(self.T_k)
        lens = torch.tensor(self.lens)
        pad = j[None, :] < lens[:, None]
        if variant == "pad":
            return pad.float()
        if variant == "pad_sec":
            npairs = lens // 2
            return (pad & ~((j[None, :] % 2 == 0) & (j[None, :] < 2 * npairs[:, None]))).float()
        assert variant == "cell"
        m = pad[torch.arange(self.b) // self.kv_group][:, None, :].repeat(1, self.T_q, 1)
        if self.secondary:
            bi, qi = torch.nonzero(self.flagged(), as_tuple=True)
            m[bi, qi, self.pri[bi, qi]] = False
        return m.float().contiguous()

    def selected(self, variant):
        """(B, Tq) the key every query must pick under `variant`."""
        if variant == "pad_sec":
            return torch.where(self.sec >= 0, self.sec, self.pri)
        if variant == "cell" and self.secondary:
            return torch.where(self.flagged(), self.sec, self.pri)
        return self.pri

    def scores(self, variant):
        """(B, H, Tq, Tk) float64 scaled scores with the additive mask of `variant` (a variant's name, a mask tensor or None)."""
        kb = torch.arange(self.b) // self.kv_group
        s = torch.einsum("bihd,bjhd->bhij", self.q + self.u, self.k[kb]) + torch.einsum("bihd,jhd->bhij", self.q + self.v, self.pos)
        s = s * self.scale
        m = self.mask(variant) if isinstance(variant, str) else variant
        if m is None:
            return s
        if m.dim() == 2:
            return s + (m[kb][:, None, None, :] == 0).double() * MASKED
        return s + (m[:, None] == 0).double() * MASKED

    def context64(self, mask):
        """(B * Tq, dm) float64 softmax(scores) . V under an arbitrary mask."""
        kb = torch.arange(self.b) // self.kv_group
        ctx = torch.einsum("bhij,bjhd->bihd", torch.softmax(self.scores(mask), -1), self.val[kb])
        return ctx.reshape(self.b * self.T_q, self.dm)

    def expected(self, variant):
        """-> (ctx (B * Tq, dm) bf16: the selected V rows, lse (B, H, Tq) float64, sel (B, Tq), off (B, H, Tq) off-target mass)."""
        sel = self.selected(variant)
        s = self.scores(variant)
        lse = torch.logsumexp(s, -1)
        at = torch.gather(s, 3, sel[:, None, :, None].expand(-1, self.heads, -1, 1))[..., 0]
        # the off-target mass as a sum over the other keys (1 - p_target would bottom out at 1e-16)
        others = s.clone()
        others.scatter_(3, sel[:, None, :, None].expand(-1, self.heads, -1, 1), -math.inf)
        off = torch.exp(torch.logsumexp(others, -1) - lse) if self.T_k > 1 else torch.zeros_like(lse)
        assert bool((at >= others.max(-1).values).all())
        kb = (torch.arange(self.b) // self.kv_group)[:, None].expand(-1, self.T_q)
        ctx = self.val[kb, sel]  # (B, Tq, H, 64)
        return ctx.reshape(self.b * self.T_q, self.dm).to(torch.bfloat16), lse, sel, off


def _flip(code, rng, amplitude):
    """`code` (..., 64) with FLIPS signs flipped, at positions drawn per row."""
    out = code.copy()
    flat = out.reshape(-1, DK)
    for r in range(flat.shape[0]):
        at = rng.choice(DK, FLIPS, replace=False)
        flat[r, at] = -flat[r, at]
    return out


def selector_case(b, T_q, T_k, heads, lens, perm, carrier, amplitude, secondary=False, kv_group=1, scale=None, seed=0):
    """One-hot attention inputs (see the module docstring).  lens: valid keys per key batch (B / kv_group of them); perm: one of PERMS;
    carrier: where the code lives - "k" (pos = 0), "pos" (k = 0: pins the pos row index and that pos is shared by the batch) or
    "k+bias" (u, v != 0, the query stored as code - u, and a +-1/8 pattern in pos that only the (q + v) half sees).
    secondary: key 2m + 1 repeats the code of key 2m with FLIPS signs flipped, and the targets are the even keys 2m with 2m + 1 < len -
    with the primary masked the secondary wins.  Asserts the one-hot condition for every mask variant of the case."""
    assert b % kv_group == 0 and len(lens) == b // kv_group and all(1 <= n <= T_k for n in lens)
    assert perm in PERMS and carrier in CARRIERS and (carrier == "k" or (T_q == T_k and kv_group == 1))
    bk = b // kv_group
    scale = 1.0 / math.sqrt(DK) if scale is None else scale
    rng = np.random.RandomState([seed, b, T_q, T_k, heads, PERMS.index(perm), CARRIERS.index(carrier), int(secondary)])
    shared = carrier == "pos"  # one code table for the whole batch
    code = rng.choice([-1.0, 1.0], size=(1 if shared else bk, T_k, heads, DK)) * amplitude
    if secondary and T_k > 1:
        npair = T_k // 2
        code[:, 1:2 * npair:2] = _flip(code[:, 0:2 * npair:2], rng, amplitude)
    code = np.broadcast_to(code, (bk, T_k, heads, DK))
    pri = np.zeros((b, T_q), np.int64)
    sec = np.full((b, T_q), -1, np.int64)
    for bi in range(b):
        n = lens[bi // kv_group]
        if secondary and n >= 2:
            pri[bi] = 2 * permutation(perm, n // 2, T_q)
            sec[bi] = pri[bi] + 1
        else:
            pri[bi] = permutation(perm, n, T_q)
        assert pri[bi].max() < n and sec[bi].max() < n
    qcode = np.stack([code[bi // kv_group, pri[bi]] for bi in range(b)])  # (B, Tq, H, 64)
    zeros_k = np.zeros((bk, T_k, heads, DK))
    u = np.zeros((heads, DK))
    v = np.zeros((heads, DK))
    if carrier == "k":
        q, k, pos = qcode, code, zeros_k[0]
    elif carrier == "pos":
        q, k, pos = qcode, zeros_k, code[0]
    else:
        quarters = np.array([-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0])
        u, v = rng.choice(quarters, size=(heads, DK)), rng.choice(quarters, size=(heads, DK))
        q, k = qcode - u, code
        pos = rng.choice([-0.125, 0.125], size=(T_k, heads, DK))
    # V: distinct for every (batch, key, head) - the first four features spell the row's number in base 128 - and bf16-exact in [1, 2)
    m = rng.randint(0, 128, size=(bk, T_k, heads, DK))
    ident = np.arange(bk * T_k * heads).reshape(bk, T_k, heads)
    for d in range(4):
        m[..., d] = (ident // 128 ** d) % 128
    val = 1.0 + m / 128.0
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # noqa: E731
    case = SelectorCase(b=b, T_q=T_q, T_k=T_k, heads=heads, lens=list(lens), perm=perm, carrier=carrier, amplitude=amplitude,
                        secondary=secondary, kv_group=kv_group, scale=scale, q=t(q), k=t(k), pos=t(pos), val=t(val), u=t(u), v=t(v),
                        pri=torch.from_numpy(pri), sec=torch.from_numpy(sec))
    # ---- the conditions the tests rest on
    for name in ("q", "k", "pos", "val", "u", "v"):
        x = getattr(case, name)
        assert torch.equal(bf16_round(x), x), name                                  # exact in bf16 as stored
    assert torch.equal(bf16_round(case.q + case.u), case.q + case.u) and torch.equal(bf16_round(case.q + case.v), case.q + case.v)
    assert float(case.val.min()) >= 1.0 and float(case.val.max()) < 2.0
    flat = case.val.reshape(-1, DK)
    assert len({tuple(r) for r in flat[:, :4].tolist()}) == flat.shape[0]           # V rows distinct
    keyed = case.k + case.pos[None]                                                  # what tells keys apart, per head
    for gap in (16, 64, 128):
        if T_k > gap:
            assert bool((keyed[:, gap:] != keyed[:, :-gap]).any(-1).all()), gap     # keys a tile apart differ in EVERY head
    # every partial sum of a score is an integer multiple of 2^-6 below 2^17: exact in float32 whatever the summation order
    assert 128 * (float(case.q.abs().max()) + 2) * float(max(case.k.abs().max(), case.pos.abs().max())) < 2 ** 17
    for variant in case.variants():
        off = case.expected(variant)[3]
        assert float(off.max()) <= OFF_MASS, (variant, float(off.max()))
    return case


# the shapes of test_attention_exact_gpu.py
RELPOS_T = (1, 15, 16, 17, 63, 64, 65, 96, 97, 128, 129, 224, 225, 301)
RELPOS_SHAPES = [(3, T, 4) for T in RELPOS_T] + [(3, 97, 8)]
RELPOS_AMPLITUDE = 4.0
DECODER_SHAPES = ((1, 1), (1, 65), (32, 320), (33, 321), (64, 64), (65, 1088), (31, 63))
DECODER_B = 4
DECODER_AMPLITUDE = 16.0  # 1 / d_k scaling: the secondary lies 2 * FLIPS * 16^2 / 64 = 32 below its primary, noise (sd 32) 224 below


def relpos_selector_cases(b, T, heads):
    for perm in PERMS:
        for carrier in CARRIERS:
            for secondary in (False, True):
                yield selector_case(b, T, T, heads, relpos_lens(b, T), perm, carrier, RELPOS_AMPLITUDE, secondary=secondary)


def decoder_lens(bk, lk):
    return [lk, max(1, lk - lk // 3), max(1, lk // 2), 1][:bk]


def decoder_selector_cases(lq, lk, kv_group=1):
    bk = DECODER_B // kv_group
    for perm in PERMS:
        for secondary in (False, True):
            yield selector_case(DECODER_B, lq, lk, 4, decoder_lens(bk, lk), perm, "k", DECODER_AMPLITUDE, secondary=secondary,
                                kv_group=kv_group, scale=1.0 / DK)


# ---- comparators --------------------------------------------------------------------------------------------------------------------
def row_floor(ref):
    """2^-6 of the median non-zero row norm: rows that are structurally zero (dk / dv of keys every query masks) are judged on an
    absolute scale."""
    n = ref.double().reshape(ref.shape[0], -1).norm(dim=1)
    nz = n[n > 1e-12]  # (float64 autograd leaves 1e-17 where the gradient is zero)
    # no row at all (T = 1: a softmax over one key passes no gradient to q, k, pos): 2^-6 absolute - the inputs have unit scale
    return 2.0 ** -6 * (float(nz.median()) if nz.numel() else 1.0)


def rowwise_err(got, ref, floor=None):
    """-> (err (rows,) = ||got_i - ref_i|| / max(||ref_i||, floor), index of the worst row)."""
    got = got.double().cpu().reshape(got.shape[0], -1)
    ref = ref.double().reshape(ref.shape[0], -1)
    floor = row_floor(ref) if floor is None else floor
    err = (got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(floor)
    return err, int(err.argmax())


def worst(got, ref):
    err, at = rowwise_err(got, ref)
    return float(err[at]), at


def old_rel(got, want):
    """The whole-tensor metric of test_train_kernels_gpu.py."""
    return float((got.float().cpu() - want).norm() / (want.norm() + 1e-30))


# ---- gradient cases: rel-pos attention ----------------------------------------------------------------------------------------------
RELPOS_GRAD_SHAPES = ((3, 1, 4), (3, 17, 4), (3, 65, 4), (3, 97, 4), (2, 129, 4), (2, 65, 8))
DECODER_GRAD_SHAPES = ((1, 1, 0), (33, 320, 1), (65, 321, 1), (64, 64, 2), (97, 97, 2))
GRAD_FACTOR = 4.0      # kernel's worst row <= 4 x the rounded reference's worst row
X32_ROW_TOL = 2e-5     # the float32 forms: the file's float32 tolerance, per row


def chunk_mask(pad, T, size=8, left=2):
    """(B, T, T): the streaming configuration's chunk mask (chunks of `size`, `left` chunks of history) with the padding folded in."""
    idx = torch.arange(T)
    chunk = ((idx[None, :] // size) <= (idx[:, None] // size)) & ((idx[None, :] // size) >= (idx[:, None] // size) - left)
    return (chunk[None] & (pad[:, None, :] > 0)).float().contiguous()


def relpos_grad_inputs(b, T, heads, chunked, lens=None, qkv_scale=1.6, seed=None):
    """Gaussian inputs as test_attention_backward's, the q / k / v scale raised so that a row has only a few effective keys."""
    g = torch.Generator().manual_seed(1000 * T + 10 * heads + int(chunked) if seed is None else seed)
    dm = heads * DK
    bf = lambda x: x.to(torch.bfloat16)  # noqa: E731
    inp = dict(b=b, T=T, heads=heads, qkv=bf(torch.randn(b * T, 3 * dm, generator=g) * qkv_scale),
               pos=bf(torch.randn(T, dm, generator=g) * 0.8), u=0.3 * torch.randn(heads, DK, generator=g),
               v=0.3 * torch.randn(heads, DK, generator=g), dctx=bf(torch.randn(b * T, dm, generator=g)),
               dpos0=torch.randn(T, dm, generator=g), du0=torch.randn(heads, DK, generator=g), dv0=torch.randn(heads, DK, generator=g))
    lens = torch.tensor(relpos_lens(b, T) if lens is None else lens)
    pad = (torch.arange(T)[None, :] < lens[:, None]).float()
    inp["lens"] = lens
    inp["mask"] = chunk_mask(pad, T) if chunked else pad
    return inp


def _mask_add(mask):
    if mask is None:
        return 0.0
    if mask.dim() == 2:
        return (mask[:, None, None, :] == 0).double() * MASKED
    return (mask[:, None] == 0).double() * MASKED


def _relpos_split(inp):
    b, T, h = inp["b"], inp["T"], inp["heads"]
    dm = h * DK
    x = inp["qkv"].double()
    q, k, vv = (x[:, i * dm:(i + 1) * dm].reshape(b, T, h, DK) for i in range(3))
    return q, k, vv, inp["pos"].double().reshape(T, h, DK)


def relpos_float64(inp, mask="own"):
    """float64 autograd of the exact formulas on the bf16 inputs -> ctx, lse, dq, dk, dv (B * T, dm), dpos (T, dm), du, dbv (H, 64):
    the gradients alone (what the kernels ADD to their dpos / du / dv buffers)."""
    mask = inp["mask"] if isinstance(mask, str) else mask
    b, T, h = inp["b"], inp["T"], inp["heads"]
    q, k, vv, p = (t.clone().requires_grad_() for t in _relpos_split(inp))
    u, v = inp["u"].double().requires_grad_(), inp["v"].double().requires_grad_()
    s = (torch.einsum("bihd,bjhd->bhij", q + u, k) + torch.einsum("bihd,jhd->bhij", q + v, p)) / math.sqrt(DK) + _mask_add(mask)
    ctx = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), vv).reshape(b * T, h * DK)
    ctx.backward(inp["dctx"].double())
    flat = lambda t: t.grad.reshape(b * T, h * DK)  # noqa: E731
    return dict(ctx=ctx.detach(), lse=torch.logsumexp(s.detach(), -1), dq=flat(q), dk=flat(k), dv=flat(vv),
                dpos=p.grad.reshape(T, h * DK), du=u.grad, dbv=v.grad)


def rounded_reference_relpos(inp, mask="own"):
    """The rel-pos backward in float64 with the roundings of attention_bwd.hip (and of the forward that feeds it): Q' = bf16(q + u) |
    bf16(q + v); the scaled, masked scores and the log-sum-exp are float32; the context the row term D is taken from is bf16; P and
    scale * dS are rounded to bf16 before the products that contract over them (dV = P^T dO, dK' = dS^T Q', dQ' = dS K'); dP and D are
    float32 sums; dq, dk, dv are stored as bf16, dpos / du / dv stay float32 sums.  NOT modelled: the kernels' summation order, the
    hardware exp2 / rcp.
    The float32 D and dP matter on rows whose gradient is exactly zero (T = 1, one visible key): attn_bwd_kernel takes both from
    separate float32 sums and leaves their cancellation noise there, so the model carries noise of the same kind (torch's summation
    order, not the kernel's).  Only the bf16 kernels are held to this model; the float32 kernels return exact zeros on such rows."""
    mask = inp["mask"] if isinstance(mask, str) else mask
    b, T, h = inp["b"], inp["T"], inp["heads"]
    scale = 1.0 / math.sqrt(DK)
    q, k, vv, p = _relpos_split(inp)
    u, v = inp["u"].double(), inp["v"].double()
    qu, qv = bf16_round(f32_round(q + u)), bf16_round(f32_round(q + v))
    s = f32_round(torch.einsum("bihd,bjhd->bhij", qu, k) + torch.einsum("bihd,jhd->bhij", qv, p))
    s = f32_round(f32_round(s * scale) + _mask_add(mask))
    lse = f32_round(torch.logsumexp(s, -1))
    P = torch.exp(f32_round(s - lse[..., None]))
    dO = inp["dctx"].double().reshape(b, T, h, DK)
    ctx = bf16_round(torch.einsum("bhij,bjhd->bihd", P, vv))
    # (float32 sums, as the kernels': where the gradient vanishes - a row with one visible key has dP = D - what is left is their noise)
    D = (dO.float() * ctx.float()).sum(-1).double().permute(0, 2, 1)      # (B, H, T)
    dP = torch.einsum("bihd,bjhd->bhij", dO.float(), vv.float()).double()
    Pb, G = bf16_round(P), bf16_round(P * (dP - D[..., None]) * scale)
    flat = lambda t: t.reshape(b * T, h * DK)  # noqa: E731
    dQu, dQv = torch.einsum("bhij,bjhd->bihd", G, k), torch.einsum("bhij,jhd->bihd", G, p)
    return dict(ctx=flat(ctx), lse=lse, dq=flat(bf16_round(dQu + dQv)), dk=flat(bf16_round(torch.einsum("bhij,bihd->bjhd", G, qu))),
                dv=flat(bf16_round(torch.einsum("bhij,bihd->bjhd", Pb, dO))),
                dpos=f32_round(torch.einsum("bhij,bihd->jhd", G, qv)).reshape(T, h * DK), du=f32_round(dQu.sum((0, 1))),
                dbv=f32_round(dQv.sum((0, 1))))


# ---- gradient cases: the decoder's attention ----------------------------------------------------------------------------------------
def decoder_grad_inputs(lq, lk, mode, b=3, heads=4, k_scale=8.0):
    """Gaussian inputs and masks as test_decoder_attention_long_sources', the key scale raised (a few effective keys per row)."""
    g = torch.Generator().manual_seed(lq * 1000 + lk + 7)
    dm = heads * DK
    bf = lambda x: x.to(torch.bfloat16)  # noqa: E731
    inp = dict(b=b, lq=lq, lk=lk, heads=heads, mode=mode, scale=1.0 / DK, q=bf(torch.randn(b * lq, dm, generator=g)),
               k=bf(torch.randn(b * lk, dm, generator=g) * k_scale), v=bf(torch.randn(b * lk, dm, generator=g)),
               dctx=bf(torch.randn(b * lq, dm, generator=g)))
    if mode == 1:
        mask = torch.ones(b, lk)
        mask[1, lk - lk // 3:] = 0
        mask[2, lk // 2:] = 0
    elif mode == 2:
        mask = torch.tril(torch.ones(lq, lk))[None].repeat(b, 1, 1).contiguous()
        if lk > 5:
            mask[2, :, lk - 5:] = 0
    else:
        mask = None
    inp["mask"] = mask
    return inp


def _decoder_split(inp):
    b, lq, lk, h = inp["b"], inp["lq"], inp["lk"], inp["heads"]
    return (inp["q"].double().reshape(b, lq, h, DK), inp["k"].double().reshape(b, lk, h, DK), inp["v"].double().reshape(b, lk, h, DK))


def decoder_float64(inp, mask="own"):
    """float64 autograd -> probs (B, H, Lq, Lk), ctx, dq (B * Lq, dm), dk, dv (B * Lk, dm)."""
    mask = inp["mask"] if isinstance(mask, str) else mask
    b, lq, lk, h = inp["b"], inp["lq"], inp["lk"], inp["heads"]
    q, k, v = (t.clone().requires_grad_() for t in _decoder_split(inp))
    probs = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * inp["scale"] + _mask_add(mask), -1)
    ctx = torch.einsum("bhij,bjhd->bihd", probs, v).reshape(b * lq, h * DK)
    ctx.backward(inp["dctx"].double())
    return dict(probs=probs.detach(), ctx=ctx.detach(), dq=q.grad.reshape(b * lq, -1), dk=k.grad.reshape(b * lk, -1),
                dv=v.grad.reshape(b * lk, -1))


def rounded_reference_decoder(inp, mask="own", staged_limit=320):
    """mha_small_bwd in float64 with the roundings of decoder_kernels.hip: the probabilities arrive as float32 and the context as
    bf16 (for the row term D); up to `staged_limit` keys (the matrix-core form) P and dS / d_k are rounded to bf16 before dV = P^T dO,
    dK = dS^T Q and dQ = dS K, and the forward rounded P before P V; beyond it the products run on the float32 values; dq, dk, dv
    are stored as bf16.  NOT modelled: the summation order, the hardware exp / rcp, the bf16 rounding of the running dk / dv between
    the 32-row query tiles.  D and dP are float32 sums for the sake of the matrix-core form (D an fmaf chain, dP an MFMA): on a row
    with one visible key it leaves their cancellation noise where the gradient is zero, as attn_bwd_kernel does."""
    mask = inp["mask"] if isinstance(mask, str) else mask
    b, lq, lk, h = inp["b"], inp["lq"], inp["lk"], inp["heads"]
    q, k, v = _decoder_split(inp)
    staged = lk <= staged_limit
    s = f32_round(f32_round(f32_round(torch.einsum("bihd,bjhd->bhij", q, k)) * inp["scale"]) + _mask_add(mask))
    P = f32_round(torch.softmax(s, -1))
    dO = inp["dctx"].double().reshape(b, lq, h, DK)
    ctx = bf16_round(torch.einsum("bhij,bjhd->bihd", bf16_round(P) if staged else P, v))
    D = (dO.float() * ctx.float()).sum(-1).double().permute(0, 2, 1)  # (float32 sums, as the kernels')
    G = f32_round(P * (torch.einsum("bihd,bjhd->bhij", dO.float(), v.float()).double() - D[..., None]) * inp["scale"])
    Pm, Gm = (bf16_round(P), bf16_round(G)) if staged else (P, G)
    return dict(probs=P, ctx=ctx.reshape(b * lq, -1), dq=bf16_round(torch.einsum("bhij,bjhd->bihd", Gm, k)).reshape(b * lq, -1),
                dk=bf16_round(torch.einsum("bhij,bihd->bjhd", Gm, q)).reshape(b * lk, -1),
                dv=bf16_round(torch.einsum("bhij,bihd->bjhd", Pm, dO)).reshape(b * lk, -1))
