"""Inputs, references, comparators and planted defects of the inference conv-module kernel tests (test_convmodule_cases_cpu.py,
test_convmodule_exact_gpu.py).  Nothing here needs a device.  The method is that of gemm_cases.py, packed_cases.py and
train_kernel_cases.py: operands whose float32 results do not depend on the order of the sums, guard-banded windows, derived
per-element intervals where a result is not exact.

FORMS (C = 256 unless noted), each one launch:
  "mid"    ma_convmodule_mid_bf16       convmodule_mid_kernel       y (B T, 2 C) bf16 -> h (B T, C) bf16; any C % 8 == 0, k <= 31
  "pw2"    ma_convmid_pw2_bf16          convmid_pw2_kernel          y -> x += mask (h W2^T + b2), in place
  "cm"     ma_convmodule_bf16           convmodule_kernel<false>    a (B T, 256) bf16 -> y = a W1^T + b1 -> ... x in place
  "oproj"  ma_attn_out_convmodule_bf16  convmodule64_kernel, or convmodule_kernel<true> under MINDAUDIO_AMD_CONVMOD=t32:
           x' = x + ctx Wo^T + bo, a = bf16(LN(x') mask), x_out = x' + mask (h W2^T + b2)
with glu = v sigmoid(g) of the halves (v | g) of y (rounded to bf16 in "cm" and "oproj", kept in float32 in "mid" and "pw2"), zero
outside the utterance, acc = sum_j w[c][j] glu[t + j - k / 2, c] (a chain of fused multiply-adds in the order of j),
z = acc bn_scale[c] + bn_shift[c], h = bf16(z sigmoid(z)).  Both sigmoids are rcp(1 + exp2(-log2 e . )), the chain gemm_cases.act_bound
was derived for.  model() states all of this once, in float64 or in float32 in the kernels' order, with one planted defect.
(train_kernel_cases.convmid_fwd_ref states the GLU and the depthwise sum of the TRAINING kernels; it knows neither tiles nor the
fused forms' bf16 GLU, which most defects here need, so model() has its own loop over the taps - and test_convmodule_cases_cpu.py
holds that loop, with and without the two defects both know, against convmid_fwd_ref.)

KINDS
  "sat"    every operand a small integer (taps in {0, +-1, +-1/2}, the halves only where bn_scale is even), gates >= 38: 1 + exp2(..)
           is 1 in float32 and the sigmoid 1.  bn_scale in {1, 2, 4}, bn_shift an integer, no two channels within a distance of 8
           (a thread's channel group) with the same pair: z is an integer of [16, 255], z (1 - sigmoid(z)) <= 16 e^-16 is far below
           half a bf16 step, bf16(swish(z)) == z (packed_cases' "sat" argument; Case asserts the range).  W2 = int_matrix(256, 256,
           0.5), b2, x0 small integers, masked frames INSIDE the utterances: x EQUALS the int64 evaluation.  "oproj": the target rows
           x' are 4096 balanced_rows (+-s, 128 of each sign, s in {2048 .. 12288}): mean 0 and variance s^2 in any order of the sums,
           and eps <= 4096 moves LN(x') gamma + beta = sign gamma (1 - eps / 2 s^2) + beta by less than 2 * 4096 / (2 * 2048^2) =
           4.9e-4 towards beta, |beta| > |gamma|: it rounds to the bf16 integer sign gamma + beta at both eps of LN_EPS.  ctx, Wo,
           bo are integers and x = x' - (ctx Wo^T + bo) in int64, so x', a and x_out are exact - and x' reaches the epilogue
           through the row rotation of the 64-frame kernel.
  "route"  one power-of-two impulse per channel in the input of the depthwise step, at route_positions: the last frame of
           utterance 0 and the first of utterance 2 around an all-zero utterance, the frames 15 | 16, 31 | 32, 63 | 64, T - 1 and the
           outermost halo frames of the tile edges.  w[c][j] = 2^-(j + c mod 5), bn_scale a power of two, bn_shift 0 in every third
           channel (z a power of two >= 64, or 0: every tap readable) and 64 or 128 in the others (z an exact float32 number >= 64,
           h = its bf16 rounding to nearest even: for z >= 32 the kernel's sigmoid is exactly 1).  W2 = the one-hot packed_cases.PI.
           x equals the float64 evaluation rounded where the kernel rounds; the middle utterance is the bare BatchNorm path.
           "mid", "pw2", "cm": channel c has its impulse 2 or 4 at entry c mod 17, in y or (through a one-hot W1) in a.
           "oproj": a is a LayerNorm output and never 0, so the impulse is built from its two values.  Column i = p1[c] of x' has
           the baseline sign -1 (blocks of 16 channels alternate: route_base_sign) in every frame but the channel's impulse frame,
           where it has the other one; W1 is one-hot, v[c] = a[p1[c]] + b1[c] with b1[c] = -(beta_i + base gamma_i): v is 0 at the
           baseline and -2 base gamma_i = +-2 or +-4 at the impulse (bn_scale carries the sign -base, so z >= 64 as before).  Entry
           route_class(c) of the first 16 positions holds 16 channels, 8 of each baseline sign: every row keeps 128 entries of each
           sign, and x' (4096 times +-s as in "sat"), a and x_out are exact at both eps.
  "glu"    v integers of [32, 127], g integers of [-3, 8], one centre tap 1, bn_scale 16, bn_shift 0, one-hot W2: z = 16 glu >= 24,
           Swish is the identity after rounding, x = fl32(x0 + 16 h), h in bf16_interval(v sigmoid(g), |v sigmoid(g)| (rho(g) + u)).
  "swish"  gates 40, z = glu + bn_shift an integer of [-12, 12], one-hot W2: h in bf16_interval(act64(z), act_bound(z)).
           "oproj" with eps = 4096 runs on 64 balanced_rows instead: LN(x') is then sign gamma s / sqrt(s^2 + 4096) + beta, no
           integer, and a = its bf16 rounding wherever packed_cases.ln_bound leaves a single bf16 number (Case asserts that it does
           everywhere): a LayerNorm without eps shows here.
Rounding is monotone, so an output lies in [fl32(x0 + lo), fl32(x0 + hi)].  Case.reference() asserts per case that at most
MULTI_CAP of the intervals hold more than one bf16 number.

OLD CRITERION (test_conformer_ops_gpu.py::test_convmodule_one_launch: max |x - ref| <= 2^-7 max |branch| on Gaussian inputs with
bn_scale = 1 + 0.1 N(0, 1)), on that test's own inputs at its five shapes (OLD_SHAPES), error of model() / tolerance (<= 1 passes):
                                                           (3, 249, 15)  (2, 33, 7)  (5, 64, 15)  (1, 5, 3)  (2, 32, 15)
    no defect                                                  0.14         0.11        0.14        0.05       0.12
    bn_swap_pair (channels 10 and 11 exchange scale, shift)    0.78         0.56        0.79        0.26       0.45     ACCEPTED
    taps_flipped_group (channels 8 .. 15)                     17.85        12.97       16.33        5.65      15.04     rejected
    bn_xor1 (every channel reads its neighbour's pair)        12.78        11.26       13.24        9.66      12.46     rejected
The swap of one pair of channels passes the old test (of the pairs of group 1, (10, 11) and (14, 15) pass at every shape, (8, 9) and
(12, 13) at some).  Reversed taps do not: even in a single channel the maximum over the tensor is 5 to 11 times the tolerance - an
element-wise estimate (2e-3 against 2e-2) holds for the typical element, not for the largest of 2 e5.  OLD_RATIOS holds the table;
test_convmodule_cases_cpu.py measures it again and asserts it to 2 digits.
"""
import types

import torch

import gemm_cases as G
import packed_cases as P
import train_kernel_cases as TK

U = G.U
C256 = 256
FORMS = ("mid", "pw2", "cm", "oproj")
KINDS = ("sat", "route", "glu", "swish")
FUSED = ("cm", "oproj")
LN_EPS = (4096.0, 1e-5)          # test_packed_exact_gpu.LN_EPS
MULTI_CAP = 0.02
TS = (1, 5, 31, 32, 33, 63, 64, 65, 129)
KS = (1, 3, 7, 15)
# T = 5 < the halo of k = 15; one frame past each tile size; two 64-frame tiles + 1
SHAPES = tuple((3, T, k) for T in TS for k in KS)
BIG_SHAPE = (40, 65, 15)
MID_EXTRA = ((3, 33, 31, 256), (3, 65, 15, 264), (3, 5, 31, 264))   # (B, T, k, C): k = 31 and a second channel block of 8 channels
OLD_TOL = 2.0 ** -7
OLD_SHAPES = ((3, 249, 15), (2, 33, 7), (5, 64, 15), (1, 5, 3), (2, 32, 15))
OLD_RATIOS = {None: (0.14, 0.11, 0.14, 0.05, 0.12), "bn_swap_pair": (0.78, 0.56, 0.79, 0.26, 0.45),
              "taps_flipped_group": (17.85, 12.97, 16.33, 5.65, 15.04), "bn_xor1": (12.78, 11.26, 13.24, 9.66, 12.46)}
SWAP_PAIR = (10, 11)
TAPS_GROUP = slice(8, 16)

# defect -> the forms it can occur in (None: all)
DEFECTS = {
    "taps_flipped": None, "taps_flipped_group": None, "halo_crosses_utterance": None, "halo_short": None,
    "nbr_last_zero": None, "nbr_first_zero": None, "last_tile_dropped": None, "bn_xor1": None, "bn_plus4": None, "bn_swap_pair": None,
    "glu_swapped": None, "masked_glu_zeroed": FUSED, "out_of_utt_glu_b1": FUSED, "b2_unmasked": ("pw2", "cm", "oproj"),
    "mask_on_xprime": ("oproj",), "xprime_rot": ("oproj",), "ln_no_eps": ("oproj",), "ln_unmasked": ("oproj",),
}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randint(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


def _perm(n, seed):
    return torch.randperm(n, generator=_gen(seed))


def _pm(shape, seed):
    return torch.randint(0, 2, shape, generator=_gen(seed)).float() * 2 - 1


def _r32(x):
    return x.float().to(x.dtype)


def _bf(x):
    return x.float().bfloat16().to(x.dtype)


def sigmul(v, g):
    """v sigmoid(g): float64 exactly, float32 by the kernels' chain."""
    if v.dtype == torch.float64:
        return v * torch.sigmoid(g)
    return v * (1.0 / (1.0 + torch.exp2(g * torch.tensor(-1.4426950408889634, dtype=torch.float32))))


def route_positions(T, half):
    """(utterance, frame) of the impulse of channel c: entry c mod 17 ("oproj": route_class(c) of the first 16): the edges of the
    utterances, of the 32- and 64-frame tiles, and the outermost halo frame of the tiles' first and last outputs."""
    f = lambda t: max(0, min(t, T - 1))  # noqa: E731
    return ((0, T - 1), (2, 0), (0, f(15)), (2, f(16)), (0, f(31)), (2, f(32)), (0, f(63)), (2, f(64)), (2, T - 1), (0, 0),
            (0, f(32 - half)), (2, f(31 + half)), (0, f(64 - half)), (2, f(63 + half)), (0, f(1)), (2, f(T - 2)), (2, f(47)))


def route_class(c):
    """"oproj": the entry of route_positions (the first 16) that holds channel c's impulse.  Every entry holds 16 channels, one
    of each 16-channel block and 8 of each baseline sign (route_base_sign), so every row of signs stays balanced."""
    return (c // 16 + c) % 16


def route_base_sign():
    """(256,) -1 / +1: the sign of the LayerNorm column of channel c wherever the channel has no impulse."""
    return ((torch.arange(C256) // 16) % 2).float() * 2 - 1


def frame_mask(B, T):
    """1 / 0 per frame, about a fifth masked, inside the utterances (first and last frames of some utterances included)."""
    b, t = torch.arange(B)[:, None], torch.arange(T)[None, :]
    return (((7 * t + 3 * b) % 5) != 0).float().reshape(B * T)


class Case:
    def __init__(self, form, kind, B, T, ks, C=C256, eps=1e-5, seed=0):
        assert form in FORMS and kind in KINDS and ks % 2 == 1 and (C == C256 or form == "mid")
        assert not (kind == "route" and B != 3)
        self.form, self.kind, self.B, self.T, self.ks, self.C, self.eps = form, kind, B, T, ks, C, eps
        s = 1000 * seed + 64 * KINDS.index(kind)
        M, half = B * T, ks // 2
        self.mask = None if kind == "route" else frame_mask(B, T)
        self.x0 = _randint(-8, 8, (M, C256), s + 1)
        onehot = kind != "sat"
        if form != "mid":
            self.w2 = G.int_matrix(C256, C256, 0.5, s + 2)
            self.b2 = torch.zeros(C256) if kind in ("glu", "swish") else _randint(-3, 3, (C256,), s + 3)
            if onehot:
                self.w2 = torch.zeros(C256, C256)
                self.w2[torch.arange(C256), P.PI] = 1
                self.w2 = self.w2.bfloat16()
        ch = torch.arange(C)
        # ---- the input of the GLU: (v | g), directly or as a W1^T + b1 ----------------------------------------------------------
        if form == "oproj":
            scale = 4096.0 if kind in ("sat", "route") else (64.0 if eps > 1.0 else 1.0)
            xp, sign = P.balanced_rows(M, s + 4)
            if kind == "route":   # the hand-built balanced signs of the module docstring
                sign = torch.empty(M, C256)
                sign[:, _perm(C256, s + 11)] = route_base_sign().expand(M, C256)
                for c in range(C256):
                    b, t = route_positions(T, half)[route_class(c)]
                    sign[b * T + t, _perm(C256, s + 11)[c]] *= -1
                assert bool((sign.sum(1) == 0).all())
                xp = sign * P._choice((0.5, 1.0, 2.0, 3.0), M, s + 5)[:, None]
            self.xp = xp * scale
            self.gamma, self.beta = P.ln_params_exact(s + 6)
            self.ctx = G.int_matrix(M, C256, 0.25, s + 8)
            self.wo = G.int_matrix(C256, C256, 0.25, s + 9)
            self.bo = _randint(-3, 3, (C256,), s + 10)
            self.x_in = (self.xp.double() - (self.ctx.double() @ self.wo.double().T + self.bo.double())).float()
            assert bool((self.x_in.double() + (self.ctx.double() @ self.wo.double().T + self.bo.double()) == self.xp.double()).all())
            ref, bound = P.ln_bound(self.xp, self.gamma, self.beta, eps)
            lo, hi = G.bf16_interval(ref, bound)
            assert bool((lo == hi).all()), "LN(x') must round to one bf16 number everywhere"
            self.a_live = lo.float()                                   # the a of an unmasked frame
            if not (eps > 1.0 and kind != "sat"):
                assert bool((self.a_live == sign * self.gamma + self.beta).all())
            a_abs = 7
        elif form == "cm":
            a_abs = {"sat": 2, "route": 0, "glu": 0, "swish": 7}[kind]
            self.a = _randint(-a_abs, a_abs, (M, C256), s + 4) if a_abs else torch.zeros(M, C256)
            if kind == "glu":
                self.a = _randint(-3, 8, (M, C256), s + 4)
        if form in FUSED:
            p1, p2, p3 = _perm(C256, s + 11), _perm(C256, s + 12), _perm(C256, s + 13)
            w1 = torch.zeros(2 * C256, C256)
            b1 = torch.zeros(2 * C256)
            if kind == "sat":
                w1[ch, p1] = _pm((C256,), s + 14)
                if form == "cm":
                    w1[ch, p2] += _pm((C256,), s + 15)
                w1[C256 + ch, p3] = _pm((C256,), s + 16)
                b1[:C256] = _randint(1, 2, (C256,), s + 17) * _pm((C256,), s + 18)
                b1[C256:] = 48 + _randint(-3, 3, (C256,), s + 19)
            elif kind == "glu":
                w1[ch, p1] = 4
                w1[C256 + ch, p3] = 1
                if form == "cm":
                    b1[:C256] = _randint(44, 95, (C256,), s + 17)
                else:
                    b1[:C256] = 80 + _randint(-16, 16, (C256,), s + 17)
                    b1[C256:] = torch.where(self.beta[p3] < 0, 6.0, 0.0)
            else:  # route, swish: v[c] = a[p1[c]], gates 40
                w1[ch, p1] = 1
                b1[C256:] = 40
                if kind == "route" and form == "oproj":   # v = 0 at the baseline sign, -2 base gamma at the flipped one
                    b1[:C256] = -(self.beta[p1] + route_base_sign() * self.gamma[p1])
            self.w1, self.b1, self.p1 = w1.bfloat16(), b1, p1
            if kind == "route" and form == "cm":
                for c in range(C256):
                    b, t = route_positions(T, half)[c % 17]
                    self.a[b * T + t, p1[c]] = 2.0 ** (1 + c % 2)
            if form == "cm":
                self.a = self.a.bfloat16()
        else:
            y = torch.zeros(B, T, 2 * C)
            if kind == "sat":
                y[..., :C], y[..., C:] = _randint(-4, 4, (B, T, C), s + 4), 41 + _randint(-3, 3, (B, T, C), s + 5)
            elif kind == "glu":
                y[..., :C], y[..., C:] = _randint(32, 127, (B, T, C), s + 4), _randint(-3, 8, (B, T, C), s + 5)
            elif kind == "swish":
                y[..., :C], y[..., C:] = _randint(-7, 7, (B, T, C), s + 4), 40.0
            else:
                y[..., C:] = 40.0
                for c in range(C):
                    b, t = route_positions(T, half)[c % 17]
                    y[b, t, c] = 2.0 ** (1 + c % 2)
            self.y = y.view(M, 2 * C).bfloat16()
            assert bool((self.y.float() == y.view(M, 2 * C)).all())
        # ---- taps and BatchNorm ------------------------------------------------------------------------------------------------
        self.dw = torch.zeros(C, ks)
        if kind == "sat":
            self.sc = P._choice((1.0, 2.0, 4.0), C, s + 20)
            ntap = min(ks, 3)
            for i in range(ntap):
                j = (_randint(0, ks - 1, (C,), s + 21 + i)).long()
                mag = torch.where(self.sc > 1, P._choice((1.0, 0.5), C, s + 25 + i), torch.ones(C))
                self.dw[ch, j] = mag * _pm((C,), s + 29 + i)
            vmax = 9 if form == "oproj" else (6 if form == "cm" else 4)
            lo = 16 + 4 * ntap * vmax
            n = 255 - 2 * lo + 16 + 1
            assert n > 8
            self.sh = lo + (ch % n).float()
            pair = torch.stack([self.sc, self.sh], 1)
            for d in range(1, 9):
                assert not bool((pair[d:] == pair[:-d]).all(1).any()), "channels within a distance of 8 must differ in (scale, shift)"
        elif kind == "route":
            self.dw = torch.exp2(-(torch.arange(ks)[None, :] + (ch % 5)[:, None]).double()).float()
            self.sh = torch.where(ch % 3 == 0, torch.zeros(C), torch.exp2(5.0 + (ch % 3).float()))
            self.sc = torch.where(ch % 3 == 0, torch.full((C,), 2.0 ** (ks + 8)), torch.full((C,), 2.0 ** max(6, ks - 9)))
            if form == "oproj":   # the impulse of a channel with baseline + is negative: a negative scale keeps z >= 64
                self.sc = -self.sc * route_base_sign()
        elif kind == "glu":
            self.dw[:, half] = 1
            self.sc, self.sh = torch.full((C,), 16.0), torch.zeros(C)
        else:
            self.dw[:, half] = 1
            self.sc, self.sh = torch.ones(C), _randint(-5, 5, (C,), s + 20)
            # no z = 0 (its interval holds +-tiny, two numbers): move the value, or where LayerNorm fixes the values, the shift
            if form == "oproj":
                for c in range(C):
                    taken = set((-self.a_live[:, p1[c]]).tolist()) | {0.0}
                    while float(self.sh[c]) in taken:
                        self.sh[c] = (self.sh[c] + 6) % 11 - 5
            elif form == "cm":
                av = self.a.float()[:, p1]
                av[av + self.sh == 0] += 1
                self.a = torch.zeros(M, C256).index_copy_(1, p1, av).bfloat16()
            else:
                yv = self.y[:, :C].float()
                yv[yv + self.sh == 0] += 1
                self.y[:, :C] = yv.bfloat16()
        self._ref = None

    # ---- conditions and references ---------------------------------------------------------------------------------------------
    def stages(self):
        """(v, g, glu, z) of the float64 model: what the conditions of the kinds speak about."""
        return model(self, want="stages")

    def reference(self):
        """{"want": tensor} for the exact kinds, {"lo", "hi", "multi"} for the interval kinds, in the output's dtype; computed once.
        Asserts the conditions the kind rests on."""
        if self._ref is not None:
            return self._ref
        v, g, glu, z = self.stages()
        is_int = lambda x: bool((x == x.round()).all())  # noqa: E731
        if self.kind == "sat":
            assert is_int(v) and is_int(g) and float(g.min()) >= 38 and float(v.abs().max()) <= 16
            assert is_int(z) and float(z.min()) >= 16 and float(z.max()) <= 255, (float(z.min()), float(z.max()))
            assert float(G.act_bound(z, G.ACT_SWISH).div(G.bf16_step(z)).max()) < 0.25   # bf16(swish(z)) == z
            want = model(self)
            if self.form != "mid":   # the int64 evaluation
                m = self.mask.long()[:, None]
                res = (self.xp if self.form == "oproj" else self.x0).long()
                assert bool((want.double() == (res + m * (z.long() @ self.w2.long().T + self.b2.long())).double()).all())
            self._ref = {"want": want}
        elif self.kind == "route":
            assert float(g.min()) >= 38 and bool(((z >= 32) | (z == 0)).all()) and bool((z.float().double() == z).all())
            want = model(self)
            bare = _bf(self.sh.double())
            mid = slice(self.T, 2 * self.T)
            if self.form == "mid":
                assert bool((want[mid].double() == bare).all())
            else:
                res = (self.xp if self.form == "oproj" else self.x0)[mid].double()
                assert bool((want[mid].double() == _r32(res + _r32(bare[P.PI] + self.b2.double()))).all())
            self._ref = {"want": want}
        else:
            if self.kind == "glu":
                assert is_int(v) and is_int(g) and 32 <= float(v.min()) and float(v.max()) <= 127
                assert -3 <= float(g.min()) and float(g.max()) <= 8
                ref = v * torch.sigmoid(g)
                lo, hi = G.bf16_interval(ref, 1.001 * ref.abs() * (TK.rho_fast(g) + U) + 2.0 ** -126)
                assert float(lo.min()) * 16 >= 24
                lo, hi = lo.double() * 16, hi.double() * 16
            else:
                assert float(g.min()) >= 38 and float(z.abs().max()) <= 12 and (self.eps > 1.0 and self.form == "oproj" or is_int(z))
                assert bool((z.float().double() == z).all())
                lo, hi = G.bf16_interval(G.act64(z, G.ACT_SWISH), G.act_bound(z, G.ACT_SWISH))
                lo, hi = lo.double(), hi.double()
            lo, hi = model(self, h=lo), model(self, h=hi)
            multi = float((lo != hi).double().mean())
            assert bool((lo <= hi).all()) and multi <= MULTI_CAP, multi
            self._ref = {"lo": lo, "hi": hi, "multi": multi}
        return self._ref

    def explain(self, tile=32):
        onehot = self.kind != "sat" and self.form != "mid"

        def f(r, c, got):
            b, t = divmod(r, self.T)
            msg = "utterance %d, frame %d = tile %d, position %d of %d-frame tiles" % (b, t, t // tile, t % tile, tile)
            if onehot:
                msg += "; column %d reads channel %d" % (c, int(P.PI[c]))
                c = int(P.PI[c])
            return msg + "; channel %d = group %d, bn (%g, %g)" % (c, c // 8, float(self.sc[c]), float(self.sh[c]))
        return f


def model(c, defect=None, tile=32, dt=torch.float64, h=None, want="out"):
    """One launch of form c.form on the inputs of c: float64 (exact arithmetic, rounded where the kernels round) or float32 in the
    kernels' operation order, with one planted defect (DEFECTS; tile = the frames per workgroup the tile defects refer to).
    h: continue from this (B T, C) bf16 activation instead of computing it.  -> the output as the kernel leaves it ("mid": bf16
    (B T, C); else float32 (B T, 256); rows a defect leaves unwritten are NaN or the residual), or (v, g, glu, z) for want="stages"."""
    assert defect is None or defect in DEFECTS
    B, T, C, ks, form = c.B, c.T, c.C, c.ks, c.form
    M, half, f32 = B * T, c.ks // 2, dt == torch.float32
    m = c.mask.to(dt) if c.mask is not None else torch.ones(M, dtype=dt)
    xres = pad = None
    if form == "oproj":
        xp = c.x_in.to(dt) + (c.ctx.to(dt) @ c.wo.to(dt).T + c.bo.to(dt))
        if f32:
            ln = P.ln32(xp, c.gamma, c.beta, c.eps, use_eps=defect != "ln_no_eps")
        else:
            ln = P.ln64(xp, c.gamma, c.beta, 0.0 if defect == "ln_no_eps" else float(torch.tensor(c.eps, dtype=torch.float32)))
        a = _bf(ln if defect == "ln_unmasked" else ln * m[:, None])
        xres = xp
    elif form == "cm":
        a = c.a.to(dt)
    if form in FUSED:
        pre = a @ c.w1.to(dt).T + c.b1.to(dt)
        v, g = pre[:, :C], pre[:, C:]
        pad = _bf(sigmul(c.b1[:C].to(dt), c.b1[C:].to(dt)))
    else:
        y = c.y.to(dt)
        v, g = y[:, :C], y[:, C:]
    if xres is None:
        xres = c.x0.to(dt)
    if defect == "glu_swapped":
        v, g = g, v
    glu = sigmul(v, g)
    if form in FUSED:
        glu = _bf(glu)
        if defect == "masked_glu_zeroed":
            glu = glu * m[:, None]
    # ---- depthwise chain, BatchNorm, Swish -------------------------------------------------------------------------------------
    w = c.dw.to(dt)
    if defect == "taps_flipped":
        w = w.flip(1)
    if defect == "taps_flipped_group":
        w = w.clone()
        w[TAPS_GROUP] = w[TAPS_GROUP].flip(1)
    tt = torch.arange(T)
    t0 = tt // tile * tile
    rows = glu.reshape(B, T, C)
    flat = glu.reshape(1, M, C)
    acc = torch.zeros(B, T, C, dtype=dt)
    for j in range(ks):
        src = tt + j - half
        ok = (src >= 0) & (src < T)
        vis = torch.ones(T, dtype=torch.bool)
        if defect == "halo_short" and half:
            vis = (src > t0 - half) & (src < t0 + tile - 1 + half)
        if defect == "nbr_last_zero":
            vis = src != t0 - 1
        if defect == "nbr_first_zero":
            vis = src != t0 + tile
        if defect == "halo_crosses_utterance":
            fs = (torch.arange(B)[:, None] * T + src[None, :]).reshape(M)
            okf = ((fs >= 0) & (fs < M)).to(dt)
            term = (flat[0, fs.clamp(0, M - 1)] * okf[:, None]).reshape(B, T, C)
        else:
            term = rows[:, src.clamp(0, T - 1)] * (ok & vis).to(dt)[None, :, None]
            if defect == "out_of_utt_glu_b1" and pad is not None:
                term = term + pad[None, None, :] * (~ok).to(dt)[None, :, None]
        acc = acc + w[:, j] * term
    idx = torch.arange(C)
    if defect == "bn_xor1":
        idx = idx ^ 1
    if defect == "bn_plus4":
        idx = (idx + 4) % C
    if defect == "bn_swap_pair":
        idx[list(SWAP_PAIR)] = idx[list(SWAP_PAIR[::-1])]
    z = (acc * c.sc.to(dt)[idx] + c.sh.to(dt)[idx]).reshape(M, C)
    if want == "stages":
        return v, g, glu, z
    hh = _bf(sigmul(z, z)) if h is None else h.to(dt)
    dead = torch.zeros(M, dtype=torch.bool)
    if defect == "last_tile_dropped" and T % tile:
        dead = (tt >= T // tile * tile).repeat(B)
    if form == "mid":
        out = hh.float()
        out[dead] = float("nan")
        return out.bfloat16()
    # ---- pointwise_conv2, mask, residual: x = xres + (h W2^T + b2) mask, each step rounded to float32 ----------------------------
    br = hh @ c.w2.to(dt).T
    b2 = c.b2.to(dt)
    upd = _r32(br * m[:, None]) + b2 if defect == "b2_unmasked" else _r32(br + b2) * m[:, None]
    if defect == "xprime_rot":
        xres = xres.reshape(B, T, -1)[:, (tt ^ 8).clamp(max=T - 1)].reshape(M, -1)
    if defect == "mask_on_xprime":
        xres = xres * m[:, None]
    x = (xres + upd).float()
    x[dead] = float("nan") if form == "oproj" else c.x0[dead]
    return x


# ---- guard bands and comparators -------------------------------------------------------------------------------------------------
def ld_window(M, N, dtype, device="cpu"):
    """gemm_cases.Window of layout "pad8": the window at column 0 of rows of N + 8 elements (16-byte aligned rows, 8 canary columns)."""
    return G.Window(M, N, dtype, "pad8", device)


def compare(win, c, tile=32):
    """The window of one launch against c.reference() -> (None or a message, worst position inside a multi-valued interval).
    Exact kinds: gemm_cases.check_window for the guard bands, then train_kernel_cases.check_exact bit for bit."""
    ref = c.reference()
    dev = win.buf.device
    if "want" in ref:
        msg = G.check_window(win, ref["want"].to(dev), (tile, 8), explain=c.explain(tile))
        if msg is None:
            worst, pos = TK.check_exact(win.view, ref)
            if worst != 0:
                msg = "equal in value but not in bits (a zero's sign) at %s" % (pos,)
        return msg, 0.0
    lo, hi = ref["lo"].to(dev), ref["hi"].to(dev)
    msg = G.check_window(win, None, (tile, 8), lo=lo, hi=hi, explain=c.explain(tile))
    got, lod, hid = win.view.double(), lo.double(), hi.double()
    wide = hid > lod
    pos = float((((got - (lod + hid) / 2).abs() / ((hid - lod) / 2).clamp(min=1e-300))[wide]).max()) if bool(wide.any()) else 0.0
    return msg, pos


def model_window(c, defect=None, tile=32, dt=torch.float32):
    """What a kernel computing model(...) would leave in a guard-banded window on the CPU."""
    out = model(c, defect, tile, dt)
    win = ld_window(c.B * c.T, out.shape[1], out.dtype)
    if c.form in ("pw2", "cm"):
        win.view.copy_(c.x0)
    win.snapshot()
    keep = ~torch.isnan(out.float())   # rows a defect leaves unwritten keep the canary (out of place) or the residual
    win.view[keep] = out[keep]
    return win


# ---- the old whole-tensor criterion ----------------------------------------------------------------------------------------------
def old_convmodule_case(b=3, tt=249, ks=15):
    """test_conformer_ops_gpu.py::test_convmodule_one_launch: its random operands, restated, as the inputs of form "cm"."""
    def rand(*shape, seed, scale=1.0):
        return torch.randn(*shape, generator=_gen(seed)) * scale
    c = types.SimpleNamespace(form="cm", kind="old", B=b, T=tt, ks=ks, C=C256, eps=0.0)   # (model() reads attributes only)
    c.a = rand(b * tt, C256, seed=41).bfloat16()
    c.w1, c.b1 = rand(2 * C256, C256, seed=42, scale=1.0 / 16).bfloat16(), rand(2 * C256, seed=43, scale=0.2)
    c.dw = rand(C256, ks, seed=32, scale=0.3)
    c.sc, c.sh = 1 + 0.1 * rand(C256, seed=33), 0.1 * rand(C256, seed=34)
    c.w2, c.b2 = rand(C256, C256, seed=35, scale=1.0 / 16).bfloat16(), rand(C256, seed=36)
    c.mask = (torch.rand(b * tt, generator=_gen(37)) > 0.2).float()
    c.x0 = rand(b * tt, C256, seed=38)
    return c


def old_convmodule_ratio(c, defect=None):
    """max |model(defect) - float64 reference| / (2^-7 max |branch|): the old test passes at <= 1."""
    d = c.a.double() @ c.w1.double().T + c.b1.double()
    y = (d[:, :C256] * torch.sigmoid(d[:, C256:])).view(c.B, c.T, C256).transpose(1, 2)
    z = torch.nn.functional.conv1d(y, c.dw.double().unsqueeze(1), padding=c.ks // 2, groups=C256)
    z = z * c.sc.double()[None, :, None] + c.sh.double()[None, :, None]
    z = (z * torch.sigmoid(z)).transpose(1, 2).reshape(c.B * c.T, C256)
    branch = z @ c.w2.double().T + c.b2.double()
    ref = c.x0.double() + branch * c.mask.double()[:, None]
    return float((model(c, defect).double() - ref).abs().max()) / (OLD_TOL * float(branch.abs().max()))
