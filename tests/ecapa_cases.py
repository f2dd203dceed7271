"""Inputs, float64 references, conditions and comparators of the ECAPA kernel tests (test_ecapa_cases_cpu.py, test_ecapa_exact_gpu.py):
every launch of csrc/ecapa_kernels.hip and csrc/res2net_fused.hip except the tap convolution (gemm_cases.TapCase).  Nothing here needs
a device.  Window, check_window, bf16_interval, int_matrix, the address-case idea and U come from gemm_cases.py.

PRINCIPLE.  Operands are dyadic rationals with few significant bits, so that every float32 sum and product a kernel forms is exact
in any order, with or without FMA contraction: the sum of |terms| divided by the common lattice step stays below 2^24 (each case
computes this margin, the CPU test asserts margin < 1).  The only roundings left are the kernels' bf16 stores; the references round
to nearest even at the same points and the device must agree bit for bit (+0 == -0).  Where a transcendental, a division or a
square root intervenes its argument is exact and the output is held to bf16_interval(ref, bound), or the result is 0 or 1 exactly.

RES2NET (Res2Case, res2net_ref).  x: integers of {-2 .. 2}, half of them non-zero, on the T interior frames, zero halo rows; W of a
step: 4 to 8 entries of +-1 per output row; bias integers of -2 .. 2, bn_scale of {1, 0.5, -0.5, 0.25}, bn_shift integers of -3 .. 3
that differ between consecutive steps for every channel.  Rounding points: y_i = bf16(...) and bf16(x_{i+1} + y_i).  The lattice of a
step is read off its actual inputs (the largest 2^-k, k >= 0, that divides them all); conditions: margin < 1, >= 50 % non-zero
interior outputs per step, and (where the case has at least 1 000 interior elements per step) >= 5 % of the elements changed by the
rounding of y and >= 0.5 % by the rounding of x + y (a bf16 y plus an integer of -2 .. 2 needs a ninth bit only where the sum climbs
into the next binade with an odd last bit: about 1 % of the elements).

ASP SELECTOR (AspCase, asp_ref).  Every logit is 0 on the selected frames of a channel and -120 or -240 elsewhere: e^-120 and
2^-173 are below the smallest float32 denormal, so the weights are exactly 1 and 0 (a lane or time slice whose reference sits at
-120 before its first selected frame has its sums multiplied by exactly 0 when they meet the others).  A channel selects n of
{1, 2, 4} frames, so S0 = n, S1 / n and S2 / n are exact: the mean half of the output is exact, the std half carries the square
root and one multiply-add (std_bound: 2 u for the root, u for each of the two roundings behind it).  The frames are k-space sets
asp_kset(c, T) rotated by 3 b per utterance.  Fused kernel: logits = a1 . Wc^T with a1[t] = e_k (T <= 128) or e_{k % 64} +
e_{64 + k // 64}, k = (t + 3 b) % T, and Wc of {0, -120}; the selected set of a channel is then a product set.  Halo rows: x holds
POISON (finite, large), a1 rows of zeros and logit rows of 0 - rows that would select if they were read.  Channel groups g = c // 16
with g % 4 == 3 select from few residues mod 16, so that some frame lanes of the fused kernel never see a selected frame.

ASP BOUNDED (AspRandomCase, asp_bound): random bf16 operands, logits of standard deviation 4, float64 on the same operands.  The
logits carry no error: they are inputs (ma_asp_pool_bf16) or products of random multiples of 1/2 and 1/4 whose float32 sum over
K = 128 is exact (ma_asp_fused_bf16; x, the BatchNorm and everything behind the logits are ordinary random values).  With d the
relative error of a weighted sum,
    d = u (8 (2.1 L + 4) + T + 64),   L = 2 log2(e) max|l|:
the exponent l2 - m2 carries 3 u L (two constant products and one fused multiply-add), the exponential 2 u more, a term passes
through at most 8 such factors (its own weight, rescales, the 4-step butterfly or the slice merge) and T + 64 additions;
    |mean' - mean| <= 2.1 d A1 + 2 u |mean|,                        A1 = sum w |x| / S0
    |var' - var|   <= 2.1 d A2 + 2 |mean| e_mean + e_mean^2 + 3 u (A2 + mean^2),   A2 = sum w x^2 / S0  (the cancellation term)
    |sd' - sd|     <= e_var / sqrt(max(var, eps)) + 2 u sd,
and the BatchNorm multiply-add adds 2 u (|v scale| + |out|).  The bf16 output must lie in bf16_interval(ref, bound); the figure
printed is preimage_ratio: the distance from the reference to the nearest float32 value that rounds to the output, over the bound
(0 wherever the output is the bf16 number nearest to the reference: nearest_share).

SE (SeCase).  Integer means, W1 with four +-1 per row, integer b1: h is an exact integer vector; W2 two entries per row, b2 on a
1/32 lattice so that utterance 0 meets the pre-activation ((37 c) % 512) / 32 - 8 of channel c exactly.  gate = sigmoid(exact y):
the admissible bf16 gates are bf16_interval(sigmoid64(y), gemm_cases.act_bound).  Block: x[t] = m + a[t + 1] - a[t] with integer
a, a[0] = a[T] = 0: the frame sum is T m exactly.  out[t, c] = bf16(x g + res) for ONE admissible g per (b, c).

LINEAR, MEAN, APPLY, ADD, PACK: integer / dyadic operands, bit equality (the time mean of a T that is no power of two: the interval
of one division).
"""

import torch

import gemm_cases as G
from gemm_cases import U, Window, bf16_interval, check_window, int_matrix  # noqa: F401  (re-exported for the tests)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
POISON = 16384.0  # halo rows and pad columns of the inputs: finite, exact in bf16, far above every operand
EPS = 1e-12
EPS32 = float(torch.tensor(EPS, dtype=F32))
LOG2E = 1.4426950408889634


def rne(v):
    """float64 tensor of float32-exact values -> round to nearest even bf16, as float64."""
    return v.float().bfloat16().double()


def trunc(v):
    return G.truncate_bf16(v.float()).double()


def lattice(*tensors):
    """The largest 2^-k (k >= 0) every element of the tensors is a multiple of."""
    for k in range(0, 60):
        s = 2.0 ** k
        if all(bool(((t.double() * s) == (t.double() * s).round()).all()) for t in tensors):
            return 2.0 ** -k
    raise AssertionError("no dyadic lattice")


def embed(x2d, ld, fill=POISON, off=0):
    """A copy of the (rows, cols) tensor as a column window of a (rows, ld) buffer filled with `fill`; returns (buffer, view)."""
    buf = torch.full((x2d.shape[0], ld), fill, dtype=x2d.dtype, device=x2d.device)
    buf[:, off:off + x2d.shape[1]] = x2d
    return buf, buf[:, off:off + x2d.shape[1]]


# ---- Res2Net ---------------------------------------------------------------------------------------------------------------------------
R2_SCALES = (1.0, 0.5, -0.5, 0.25)
R2_SHAPES = [(1, 4, 2), (8, 4, 4), (9, 4, 1), (40, 4, 3), (56, 4, 2), (72, 4, 3), (375, 4, 2), (376, 4, 4), (20, 8, 3), (12, 2, 2)]  # (T, H, d)
R2_CCS = (64, 128)
R2_DEFECTS = ("taps_swapped", "dil_plus", "prev_params", "keep_late", "drop_last_row", "add_f32", "truncate")


class Res2Case:
    def __init__(self, cc, T, H, d, B=3, seed=0):
        self.cc, self.T, self.H, self.d, self.B = cc, T, H, d, B
        self.C, self.tp = 8 * cc, T + 2 * H
        g = G._gen(977 * seed + 31)
        self.x = torch.zeros(B, self.tp, self.C, dtype=BF16)
        self.x[:, H:H + T] = int_matrix(B * T, self.C, 0.5, 16 * seed + 1).view(B, T, self.C)
        K = 3 * cc
        order = torch.rand(7, cc, K, generator=g).argsort(-1)[..., :8]
        cnt = torch.randint(4, 9, (7, cc, 1), generator=g)
        sign = torch.randint(0, 2, (7, cc, 8), generator=g) * 2 - 1
        vals = (sign * (torch.arange(8) < cnt)).float()
        self.w = torch.zeros(7, cc, K).scatter_(-1, order, vals).bfloat16()
        self.bias = torch.randint(-2, 3, (7, cc), generator=g).float()
        self.scale = torch.tensor(R2_SCALES)[torch.randint(0, 4, (7, cc), generator=g)]
        base = torch.randint(0, 7, (cc,), generator=g)
        self.shift = ((base[None, :] + 3 * torch.arange(7)[:, None]) % 7 - 3).float()

    def ref(self, defect=None, site=None, stats=None):
        return res2net_ref(self.x.double(), self.w.double(), self.bias.double(), self.scale.double(), self.shift.double(), self.T,
                           self.H, self.d, defect, site, stats)


def res2net_ref(x, w, bias, sc, sh, T, H, d, defect=None, site=None, stats=None):
    """The chain of csrc/res2net_fused.hip in float64 with its rounding points; x (B, tp, 8 cc) float64 of bf16 values.  stats (a
    dict) receives the exactness margin and the shares the conditions speak of.  Defects: R2_DEFECTS (drop_last_row is applied to
    the output buffer: drop_last_row())."""
    B, tp, C = x.shape
    cc = C // 8
    rnd = trunc if defect == "truncate" else rne
    y = torch.zeros_like(x)
    y[..., :cc] = x[..., :cc]
    keep = torch.zeros(tp, dtype=F64)
    k0 = H + (1 if defect == "keep_late" else 0)
    keep[k0:k0 + T] = 1
    dd = d + 1 if defect == "dil_plus" else d
    taps = (2, 1, 0) if defect == "taps_swapped" else (0, 1, 2)
    prev = raw = None
    margin, nonzero, round_y, round_add, count = 0.0, [], 0, 0, 0
    for s in range(1, 8):
        xs = x[..., s * cc:(s + 1) * cc]
        if prev is None:
            inp = xs
        else:
            exact = xs + (raw if defect == "add_f32" else prev)
            inp = rnd(exact)
            round_add += int((inp != exact)[:, H:H + T].sum())
        pad = torch.zeros(B, tp + 2 * dd, cc, dtype=F64)
        pad[:, dd:dd + tp] = inp
        W = w[s - 1].view(cc, 3, cc)
        pb, ps, pt = bias[s - 1].clone(), sc[s - 1].clone(), sh[s - 1].clone()
        if defect == "prev_params" and s == 7:
            pb[site], ps[site], pt[site] = bias[s - 2][site], sc[s - 2][site], sh[s - 2][site]
        v = sum(pad[:, k * dd:k * dd + tp] @ W[:, taps[k]].T for k in range(3)) + pb
        raw = ((v.clamp(min=0) * ps + pt) * keep[None, :, None]).float().double()
        prev = rnd(raw)
        y[..., s * cc:(s + 1) * cc] = prev
        if stats is not None:
            lat = lattice(inp, pb)
            terms = sum(pad[:, k * dd:k * dd + tp].abs() @ W[:, k].abs().T for k in range(3)) + pb.abs()
            margin = max(margin, float(terms.max()) / lat / 2.0 ** 24,
                         float((terms * ps.abs() + pt.abs()).max()) / (lat * lattice(ps)) / 2.0 ** 24)
            nonzero.append(float((prev[:, H:H + T] != 0).double().mean()))
            round_y += int((prev != raw)[:, H:H + T].sum())
            count += B * T * cc
    if stats is not None:
        stats.update(margin=margin, nonzero=nonzero, round_y=round_y / count, round_add=round_add / (count * 6 / 7), ymax=float(y.abs().max()),
                     count=count // 7)
    return y


def drop_last_row(y, prefill, cc):
    """The defect 'last row of a partial row tile not stored': the last row of every utterance keeps what the buffer held."""
    y = y.clone()
    if y.shape[1] % 16:
        y[:, -1, cc:] = prefill
    return y


def res2_old_check(got, want, H, T):
    """The whole-tensor check of test_ecapa_gpu.py::test_res2net_fused_entry_point_against_float64."""
    err = (got - want).abs()
    return (float(err.max()) <= 4e-2 * float(want.abs().max()) and float(err.mean()) <= 2e-3 * float(want.abs().mean() + 1e-6)
            and float(got[:, :H].abs().max()) == 0.0 and float(got[:, H + T:].abs().max()) == 0.0)


# ---- attentive statistics pooling --------------------------------------------------------------------------------------------------------
ASP_SCALES = (1.0, 2.0, -1.0, 0.5)
ASP_FUSED_SHAPES = [(2, 1, 256), (2, 15, 256), (2, 16, 256), (2, 17, 512), (3, 33, 256), (2, 49, 256), (2, 64, 256), (2, 65, 256),
                    (2, 130, 256), (2, 300, 768)]  # (B, T, C)
ASP_POOL8_SHAPES = [(2, T, C) for C in (64, 192) for T in (1, 31, 32, 33, 70)]
ASP_SCALAR_SHAPES = [(2, T, C) for C in (72, 40) for T in (1, 33, 70)]  # + C = 64 with ldl % 8 != 0 (the GPU test's layout)
ASP_DEFECTS = ("swap", "std_mean_params", "frame_T", "row0", "uniform16", "no_rescale")


def asp_kset(c, T):
    """The k-space frames channel c selects: 1, 2 or 4 of them (a product set in (k % 64, k // 64) when T > 128)."""
    g = c // 16
    if g % 4 == 3:
        p0, n = (5 * g + c % 2) % T, 1 + c % 2
    else:
        p0, n = (19 * c) % T, (1, 2, 4)[c % 3]
    if T <= 128:
        offs = {1: (0,), 2: (0, 1 + 5 * (c % 3)), 4: (0, 1, 17 + c % 4, 40)}[n]
        ks = {(p0 + o) % T for o in offs}
    else:
        q0, r0 = divmod(p0, 64)
        nq = (T + 63) // 64
        if n == 1:
            ks = {p0}
        elif n == 2:
            ks = {64 * q0 + r0, 64 * q0 + (r0 + 1 + 5 * (c % 3)) % 64}
        else:
            ks = {64 * q + r for q in (q0, (q0 + 1) % nq) for r in (r0, (r0 + 17) % 64)}
        if any(k >= T for k in ks):
            ks = {p0}
    if len(ks) not in (1, 2, 4):
        ks = {p0}
    return sorted(ks)


class AspCase:
    """fused=True: a1 (B, tp, 128) and Wc (C, 128); else logits (B, tp, C).  x (B, tp, C), sc / sh (2 C) float32."""

    def __init__(self, B, T, C, H=3, fused=True):
        self.B, self.T, self.C, self.H, self.fused = B, T, C, H, fused
        tp = self.tp = T + 2 * H
        ksel = torch.zeros(T, C, dtype=torch.bool)
        for c in range(C):
            ksel[asp_kset(c, T), c] = True
        self.ksel = ksel
        t, b, c = torch.arange(T), torch.arange(B), torch.arange(C)
        k = (t[None, :] + 3 * b[:, None]) % T                       # (B, T)
        self.sel = ksel[k]                                           # (B, T, C)
        self.x = torch.full((B, tp, C), POISON, dtype=BF16)
        bb, tt, cch = b[:, None, None], t[None, :, None], c[None, None, :]
        self.x[:, H:H + T] = (((5 * bb + 3 * tt + 7 * cch + (tt * cch) % 11) % 17) - 8).to(BF16)
        S = torch.tensor(ASP_SCALES)
        self.sc = torch.cat([S[c % 4], S[(c + 1) % 4]]).float()
        self.sh = torch.cat([(c % 7) - 3, ((c + 3) % 7) - 3]).float()
        if fused:
            self.a1 = torch.zeros(B, tp, 128, dtype=BF16)            # halo rows: zeros = a logit of 0 in every channel
            a = torch.zeros(B, T, 128)
            if T <= 128:
                a.scatter_(2, k[:, :, None], 1.0)
                wc = torch.full((C, 128), -240.0)
                wc[:, :T] = torch.where(ksel.T, 0.0, -120.0)
            else:
                a.scatter_(2, (k % 64)[:, :, None], 1.0)
                a.scatter_(2, (64 + k // 64)[:, :, None], 1.0)
                wc = torch.full((C, 128), -120.0)
                for ch in range(C):
                    ks = asp_kset(ch, T)
                    A, Q = {q % 64 for q in ks}, {q // 64 for q in ks}
                    assert sorted(64 * q + r for q in Q for r in A) == ks
                    wc[ch, sorted(A)] = 0.0
                    wc[ch, [64 + q for q in sorted(Q)]] = 0.0
            self.a1[:, H:H + T] = a.to(BF16)
            self.wc = wc.to(BF16)
            self.logits = None
        else:
            lg = torch.where((tt + cch) % 3 == 0, -240.0, -120.0).expand(B, T, C).clone()
            lg[self.sel] = 0.0
            self.logits = torch.zeros(B, tp, C, dtype=BF16)          # halo rows: 0 = selected
            self.logits[:, H:H + T] = lg.to(BF16)

    def logits64(self):
        """(B, tp, C) float64, halo rows included (what a kernel that read them would see)."""
        if self.fused:
            return self.a1.double() @ self.wc.double().T
        return self.logits.double()

    def ref(self, defect=None, site=None):
        return asp_ref(self.logits64(), self.x.double(), self.sc.double(), self.sh.double(), self.T, self.H, defect=defect, site=site)

    def conditions(self):
        """Every statement of the docstring about this case's selection, as a dict of booleans / figures."""
        T, sel = self.T, self.sel
        lg = self.logits64()[:, self.H:self.H + T]
        n = sel.sum(1)
        first = sel.int().argmax(1)                                 # (B, C): first selected frame
        ntiles = (T + 15) // 16
        bounds = [f for kq in range(1, ntiles) for f in (16 * kq - 1, 16 * kq)]
        lanes_unseen = False
        for fi in range(min(T, 16) if self.C % 16 == 0 else 0):
            seen = sel[:, fi::16].any(1)                            # (B, C)
            lanes_unseen |= bool((~seen.view(self.B, -1, 16).any(2)).any())
        return dict(
            levels=bool(((lg == 0) == sel).all()) and bool((lg[~sel] <= -120).all()),
            n_ok=bool(((n == 1) | (n == 2) | (n == 4)).all()), n_kinds=sorted(set(n.flatten().tolist())),
            frame0=bool(sel[:, 0].any()), frame_last=bool(sel[:, T - 1].any()),
            boundaries=all(bool(sel[:, f].any()) for f in bounds),
            first_tiles=sorted(set((first // 16).flatten().tolist())), want_tiles=list(range(min(5, ntiles))),
            lanes_unseen=lanes_unseen)


def asp_weights(l):
    """(B, T, C) float64 logits -> weights relative to the channel's maximum; below e^-100 exactly 0, as in float32."""
    d = l - l.max(1, keepdim=True).values
    return torch.where(d < -100.0, torch.zeros_like(d), d.exp())


def asp_ref(lf, xf, sc, sh, T, H, eps=EPS32, defect=None, site=None):
    """Attentive statistics + BatchNorm in float64 on (B, tp, C) logits and x -> (out (B, 2 C), parts).  Defects: ASP_DEFECTS."""
    B, tp, C = xf.shape
    r0 = 0 if defect == "row0" else H
    n = T + 1 if defect == "frame_T" else T
    l, x = lf[:, r0:r0 + n].clone(), xf[:, r0:r0 + n]
    if defect == "uniform16":
        l[:, :16] = l.max(1, keepdim=True).values.expand(B, n, C)[:, :16]
    w = asp_weights(l)
    if defect == "no_rescale" and n >= 48:  # the frame lanes whose reference moves in tile 2 keep the sums of tiles 0 and 1
        old = torch.maximum(l[:, 0:16], l[:, 16:32])
        moved = (l[:, 32:48] - old) > 40.0 / LOG2E
        w[:, 0:16] = torch.where(moved, (l[:, 0:16] - old).exp(), w[:, 0:16])
        w[:, 16:32] = torch.where(moved, (l[:, 16:32] - old).exp(), w[:, 16:32])
    s0 = w.sum(1)
    mean, ex2 = (w * x).sum(1) / s0, (w * x * x).sum(1) / s0
    var = (ex2 - mean * mean).clamp(min=eps)
    sd = var.sqrt()
    scm, shm, scs, shs = sc[:C], sh[:C], sc[C:].clone(), sh[C:].clone()
    if defect == "std_mean_params":
        scs[site], shs[site] = scm[site], shm[site]
    out = torch.cat([mean * scm + shm, sd * scs + shs], 1)
    if defect == "swap":
        c1, c2 = site
        out[:, [c1, c2, C + c1, C + c2]] = out[:, [c2, c1, C + c2, C + c1]]
    a1 = (w * x.abs()).sum(1) / s0
    return out, dict(mean=mean, ex2=ex2, var=var, sd=sd, a1=a1, s0=s0, sc=sc, C=C)


def std_bound(out, parts):
    """Selector cases: the mean half is exact; the std half carries sqrt (2 u) and the multiply-add (u for each rounding)."""
    C, sd = parts["C"], parts["sd"]
    b = torch.zeros_like(out)
    b[:, C:] = 2 * U * (sd * parts["sc"][C:]).abs() + U * ((sd * parts["sc"][C:]).abs() + out[:, C:].abs())
    return b


def asp_old_check(got, want):
    """The whole-tensor check of test_ecapa_gpu.py::test_asp_fused_entry_point_against_float64."""
    return float((got - want).abs().max()) <= 2e-2 * float(want.abs().max()) + 1e-2


class AspRandomCase:
    def __init__(self, B, T, C, H=3, fused=True, offset=0.0, seed=0):
        self.B, self.T, self.C, self.H, self.fused, self.tp = B, T, C, H, fused, T + 2 * H
        g = G._gen(seed + 1000 * T + C)
        tp = self.tp
        self.x = torch.full((B, tp, C), POISON, dtype=BF16)
        self.x[:, H:H + T] = (torch.randn(B, T, C, generator=g) + offset).to(BF16)
        self.sc = (torch.rand(2 * C, generator=g) + 0.5).float()
        self.sh = (0.1 * torch.randn(2 * C, generator=g)).float()
        if fused:
            self.a1 = torch.zeros(B, tp, 128, dtype=BF16)
            # multiples of 1/2 and 1/4: the float32 logits are exact in any order (|l| <= 96 on a lattice of 1/8), variance 128 / 8
            self.a1[:, H:H + T] = (torch.randint(-2, 3, (B, T, 128), generator=g) / 2.0).to(BF16)
            self.wc = (torch.randint(-3, 4, (C, 128), generator=g) / 4.0).to(BF16)
        else:
            self.logits = torch.full((B, tp, C), 30.0, dtype=BF16)  # a halo row that was read would take all the weight
            self.logits[:, H:H + T] = (4.0 * torch.randn(B, T, C, generator=g)).to(BF16)

    def logits64(self):
        return self.a1.double() @ self.wc.double().T if self.fused else self.logits.double()

    def ref(self):
        out, parts = asp_ref(self.logits64(), self.x.double(), self.sc.double(), self.sh.double(), self.T, self.H)
        return out, asp_bound(out, parts, self.logits64()[:, self.H:self.H + self.T], self.T)


def asp_bound(out, parts, l, T):
    """The per-element bound of the module docstring; l (B, T, C) interior logits (exact in float32)."""
    C, mean, ex2, var, sd, sc = parts["C"], parts["mean"], parts["ex2"], parts["var"], parts["sd"], parts["sc"]
    L = 2 * LOG2E * l.abs().max(1).values
    d = U * (8 * (2.1 * L + 4) + T + 64)
    e_mean = 2.1 * d * parts["a1"] + 2 * U * mean.abs()
    e_var = 2.1 * d * ex2 + 2 * mean.abs() * e_mean + e_mean ** 2 + 3 * U * (ex2 + mean ** 2)
    e_sd = e_var / var.sqrt() + 2 * U * sd
    bm = sc[:C].abs() * e_mean + 2 * U * ((mean * sc[:C]).abs() + out[:, :C].abs())
    bs = sc[C:].abs() * e_sd + 2 * U * ((sd * sc[C:]).abs() + out[:, C:].abs())
    return torch.cat([bm, bs], 1)


def preimage_ratio(got, ref, bound):
    """max over the elements of (distance from ref to the nearest float32 value that rounds to the bf16 `got`) / bound."""
    g = got.double()
    half = G.bf16_step(g) / 2
    dist = ((g - ref).abs() - half).clamp(min=0)
    return float((dist / bound.clamp(min=1e-300)).max())


def relrms(a, ref):
    return float((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def nearest_share(got, ref):
    return float((got == ref.float().bfloat16()).double().mean())


def in_interval(got, ref, bound):
    lo, hi = bf16_interval(ref, bound)
    return (got.double() >= lo.double()) & (got.double() <= hi.double())


def multi_share(ref, bound):
    lo, hi = bf16_interval(ref, bound)
    return float((lo != hi).double().mean())


# ---- time mean, SE apply, add, pack ------------------------------------------------------------------------------------------------------
MEAN_TS = (1, 3, 4, 5, 31, 32, 33, 100)
MEAN_LAYOUTS = [(64, 72, "mean8"), (512, 528, "mean8"), (72, 80, "scalar"), (64, 68, "scalar")]  # (C, ldx, kernel)


def mean_case(B, T, C, H=2, seed=0):
    """x (B, tp, C) bf16: integers of -20 .. 20 inside, POISON halo rows -> (x, ref float64, bound)."""
    x = torch.full((B, T + 2 * H, C), POISON, dtype=BF16)
    x[:, H:H + T] = torch.randint(-20, 21, (B, T, C), generator=G._gen(seed + 100 * T + C)).to(BF16)
    ref = x[:, H:H + T].double().sum(1) / T
    bound = torch.zeros_like(ref) if T & (T - 1) == 0 else 2 * U * ref.abs()
    return x, ref, bound


def apply_case(B, T, C, H=2, seed=0):
    """x integers of -8 .. 8, gate j / 64, residual integers / 4 -> (x, gate, res (B, tp, C) bf16, want (B, tp, C) bf16)."""
    g = G._gen(seed + 10 * T + C)
    tp = T + 2 * H
    x = torch.full((B, tp, C), POISON, dtype=BF16)
    res = torch.full((B, tp, C), POISON, dtype=BF16)
    x[:, H:H + T] = torch.randint(-8, 9, (B, T, C), generator=g).to(BF16)
    res[:, H:H + T] = (torch.randint(-32, 33, (B, T, C), generator=g) / 4.0).to(BF16)
    gate = (torch.randint(0, 65, (B, C), generator=g) / 64.0).to(BF16)
    want = torch.zeros(B, tp, C, dtype=BF16)
    want[:, H:H + T] = apply_ref(x[:, H:H + T], gate, res[:, H:H + T])
    return x, gate, res, want


def apply_ref(x, gate, res):
    """bf16(x g + res): one float32 rounding of the exact value (FMA or not: the product is exact), then round to nearest even."""
    return (x.double() * gate.double()[:, None, :] + res.double()).float().bfloat16()


def add_case(rows, cols, seed=0):
    """Random bf16 pairs over 12 binades with hand-built ties in the first row -> (a, b, want)."""
    g = G._gen(seed + rows + cols)
    a = (torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, cols), generator=g).float())).to(BF16)
    b = (torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, cols), generator=g).float())).to(BF16)
    ties = torch.tensor([[256.0, 1.0], [258.0, 1.0], [-256.0, -1.0], [-258.0, -1.0], [1.0, 2.0 ** -8], [1.0078125, 2.0 ** -8],
                         [3.0, -3.0], [0.0, 0.0]])
    a[0, :8], b[0, :8] = ties[:, 0].to(BF16), ties[:, 1].to(BF16)
    return a, b, (a.float() + b.float()).bfloat16()


def pack_case(B, T, F, seed=0):
    """(B, T, F) float32 with exact ties to even and to odd neighbours among random values."""
    g = G._gen(seed + T + F)
    x = torch.randn(B, T, F, generator=g) * 3
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 2.0 ** -20 * (1 + 2.0 ** -8),
                         1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23])
    x[:, 0, :7] = ties
    x[:, -1, -7:] = ties
    return x


def pack_ref(x, H, Cpad):
    B, T, F = x.shape
    want = torch.zeros(B, T + 2 * H, Cpad, dtype=BF16)
    want[:, H:H + T, :F] = x.bfloat16()
    return want


# ---- squeeze and excitation ---------------------------------------------------------------------------------------------------------------
SE_GATE_S = (8, 24, 64, 120, 128)
SE_BLOCK = [(512, 16, 1), (512, 48, 15), (512, 128, 16), (512, 16, 17), (512, 48, 255), (512, 128, 256), (512, 16, 257), (512, 48, 300),
            (1024, 128, 1), (1024, 16, 15), (1024, 48, 16), (1024, 128, 17)]  # (C, S, T)
SE_DEFECTS = ("mean_T2H", "gate_xor1", "skip_256", "w1_row_reuse", "halo_left")


class SeCase:
    def __init__(self, C, S, B=2, T=None, H=2, seed=0):
        self.C, self.S, self.B, self.T, self.H = C, S, B, T, H
        c, b, j = torch.arange(C), torch.arange(B), torch.arange(S)
        self.mean = torch.randint(-3, 4, (B, C), generator=G._gen(seed + C + S)).to(BF16)
        w1 = torch.zeros(S, C)
        for i in range(4):
            w1[j, (13 * j + 97 * i + 5) % C] += 1.0 if i % 2 == 0 else -1.0
        self.w1 = w1.to(BF16)
        self.b1 = (6 + j % 5).float()
        w2 = torch.zeros(C, S)
        w2[c, c % S] += 1.0
        w2[c, (7 * (c // S) + 3) % S] -= 1.0
        self.w2 = w2.to(BF16)
        h0 = self.hidden(self.mean.double())[0]
        self.target = ((37 * c) % 512) / 32.0 - 8.0
        self.b2 = (self.target.double() - self.w2.double() @ h0).float()
        if T is not None:
            g = G._gen(seed + 3 * T + C + S)
            tp = T + 2 * H
            a = torch.randint(-3, 4, (B, T + 1, C), generator=g)
            a[:, 0], a[:, T] = 0, 0
            self.x = torch.full((B, tp, C), POISON, dtype=BF16)
            self.x[:, H:H + T] = (self.mean.double()[:, None, :] + (a[:, 1:] - a[:, :-1])).to(BF16)
            self.res = torch.full((B, tp, C), POISON, dtype=BF16)
            self.res[:, H:H + T] = (torch.randint(-32, 33, (B, T, C), generator=g) / 4.0).to(BF16)

    def hidden(self, mean, defect=None, site=None):
        w1 = self.w1.double()
        if defect == "w1_row_reuse":  # the last row of wave `site` (S / 8 rows per wave) computed from the row before it
            rows = self.S // 8
            w1 = w1.clone()
            w1[site * rows + rows - 1] = w1[site * rows + max(rows - 2, 0)]
        return (mean @ w1.T + self.b1.double()).clamp(min=0)

    def pre(self, mean=None, defect=None, site=None):
        """The exact pre-activation y (B, C) float64 of the gate."""
        mean = self.mean.double() if mean is None else mean
        return self.hidden(mean, defect, site) @ self.w2.double().T + self.b2.double()

    def margin(self):
        m, w1, w2 = self.mean.double().abs(), self.w1.double().abs(), self.w2.double().abs()
        h = self.hidden(self.mean.double())
        t1 = (m @ w1.T + self.b1.double().abs()).max()
        t2 = (h @ w2.T + self.b2.double().abs()).max() / lattice(self.b2)
        t3 = 0.0 if self.T is None else float(self.x[:, self.H:self.H + self.T].double().abs().sum(1).max())
        return max(float(t1), float(t2), t3) / 2.0 ** 24

    def gate_interval(self, y=None):
        y = self.pre() if y is None else y
        return bf16_interval(torch.sigmoid(y), G.act_bound(y, G.ACT_SIGMOID))

    def block_ref(self, gate):
        """out (B, tp, C) bf16 for a (B, C) bf16 gate: zero halo rows, bf16(x g + res) inside."""
        H, T = self.H, self.T
        want = torch.zeros(self.B, T + 2 * H, self.C, dtype=BF16)
        want[:, H:H + T] = apply_ref(self.x[:, H:H + T], gate, self.res[:, H:H + T])
        return want


def block_matches(got, case, lo, hi):
    """(B, C) bool: the (B, tp, C) bf16 output equals block_ref(g) on ALL rows for g = lo or g = hi of its channel."""
    ok_lo = (got == case.block_ref(lo)).all(1)
    ok_hi = (got == case.block_ref(hi)).all(1)
    return ok_lo | ok_hi


def gate_old_check(got, want):
    return float((got.double() - want).abs().max()) <= 5e-3


# ---- the embedding Linear -----------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(16, 16, 3072), (32, 48, 3072), (16, 16, 6144), (32, 48, 6144)]


def linear_hot_ks(K):
    """First and last column of every wave's K slice (K / 8) and of every 384-column block inside it."""
    kw = K // 8
    return [w * kw + blk + e for w in range(8) for blk in range(0, kw, 384) for e in (0, 383)]


def linear_address_case(N, K):
    """A one-hot at linear_hot_ks (one row each, padded to a multiple of 16 rows by repeating), W = gemm_cases.address_w."""
    ks = linear_hot_ks(K)
    M = (len(ks) + 15) // 16 * 16
    ks = torch.tensor((ks * 2)[:M])
    a = torch.zeros(M, K, dtype=BF16)
    a[torch.arange(M), ks] = 1
    w = G.address_w(torch.arange(N)[:, None], torch.arange(K)[None, :]).to(BF16)
    want = G.address_w(torch.arange(N)[None, :], ks[:, None]).float()
    return a, w, want, ks


def linear_ref(c, bias=True, defect=None, site=0):
    """float64 (exact) out of a gemm_cases.Case; defects: 'slice_dropped' (wave `site`'s K / 8 columns), 'bias_n0'."""
    a, w = c.a.double(), c.w.double()
    if defect == "slice_dropped":
        kw = c.K // 8
        a = a.clone()
        a[:, site * kw:(site + 1) * kw] = 0
    z = a @ w.T
    if bias:
        bv = c.bias.double()
        if defect == "bias_n0":
            bv = bv.view(-1, 16)[:, :1].expand(-1, 16).reshape(-1)
        z = z + bv
    return z
