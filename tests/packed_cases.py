"""Inputs, references, comparators and planted defects of the packed-weight kernel tests (test_packed_cases_cpu.py,
test_packed_exact_gpu.py): ffn_packed.hip / ffn_pc.hip, gemm_k256.hip, rows_packed.hip, conv2_packed.hip, subsample_fused.hip and the
stand-alone subsampling conv1.  Nothing here needs a device.  The method is that of gemm_cases.py (integer operands whose float32
results do not depend on the order of the sums, guard-banded output windows, derived per-element bounds where a result is not exact).

FFN, x += alpha (swish(a W1^T + b1) W2^T + b2), 64-row tiles, a wave owns the hidden units of block hb = 4 sb + wave (32 units each):
  SATURATED (FfnCase kind "sat").  a in {-2 .. 2} (or the exact LayerNorm rows below, |a| <= 7), each row of W1 eight non-zeros of
    +-1 / +-2, one per 32-wide k-step at k mod 32 = (unit + 5 kstep) mod 32, b1 = base + {-3 .. 3} (base 64, or 132 for the LayerNorm
    rows): every pre-activation y is an integer of [16, 255], y (1 - sigmoid(y)) <= 16 e^-16 = 1.8e-6 is far below half a bf16 step
    (>= 2^-4 at 16), so bf16(swish(y)) == y, an integer of 8 bits.  W2 = int_matrix(256, hidden, 0.5), b2 and x0 small integers (or
    the +-s rows), alpha in {0.5, 1}: all partial sums of the second product are integers below 2^23 and x EQUALS the int64 evaluation.
  INTERVAL (kind "act").  a, W1 sparse integers, b1 in {-3 .. 3}: y an exact integer of either sign.  W2 of pass p is one-hot,
    W2[n, 256 p + PI(n)] = 1, b2 = 0, alpha = 1: x[m, n] = fl32(x0[m, n] + h[m, 256 p + PI(n)]) with h the kernel's bf16 Swish.  Both
    kernels run the chain act_bound (gemm_cases) was derived for (t = fl(-log2 e) y, v_exp_f32, 1 +, v_rcp_f32, y r: ffn_packed.hip
    nano(), ffn_pc.hip's S job), so h lies in bf16_interval(act64(y), act_bound(y)) and, rounding being monotone, x in
    [fl32(x0 + lo), fl32(x0 + hi)].
  INPUT LAYERNORM.  A row of x0 is +-s, 128 of each sign, s in {0.5, 1, 2, 3}: mean 0, variance s^2 (exactly, in any order of the
    sums), so LN(x0) gamma + beta = sign * gamma * (1 - eps / (2 s^2) + O(1e-7)) + beta, which rounds to the bf16 integer
    sign * gamma + beta when gamma in {1, 2} and |beta| in {3, 4, 5} (no cancellation to 0).
  LAYERNORM OUTPUTS are not exact: ln_bound() below.

LAYERNORM BOUND (ln_bound; u = 2^-24, N = 256, v the stage's float32 input read back from the device or known exactly).  The kernels
(ffn_packed.hip layer_norm, ffn_pc.hip layer_norm, gemm_k256.hip) form S = sum v and Q = sum v^2 in float32, every term passing
through at most D additions (ffn_packed: 63 in a lane + 2 shuffles = 65; the other two <= 10; LN_DEPTH = 65 covers all), then
    mean = S / 256, var = max(Q / 256 - mean^2, 0), rstd = 1 / sqrtf(var + eps), out = (v - mean) rstd gamma + beta.
With g = D u / (1 - D u), g' the same for D + 1 (the squares round once more), A = mean |v|, E2 = mean v^2, mu and sigma^2 exact:
    |mean - mu| <= g A =: dm                      (the division by 256 is exact)
    |Q / 256 - E2| <= g' E2;  |fl(mean^2) - mu^2| <= (2 |mu| dm + dm^2)(1 + u) + u mu^2
    dV := |var - sigma^2| <= g' E2 + (2 |mu| dm + dm^2)(1 + u) + u mu^2 + u (sigma^2 + the former)    (the clamp at 0 only helps)
    t = fl(var + eps): |t - T| <= dV + u (T + dV) =: dT, T = sigma^2 + eps (eps the float32 value the launch passes)
    rstd: sqrtf within 2 ULP and the division within 2.5 ULP (9 u together; correctly rounded forms do better):
          relative error rho <= (1 - dT / T)^-1/2 - 1 + 9 u
    out:  |fl(v - mean) - (v - mu)| <= dm + u (|v - mu| + dm) =: d0;  two products and one sum round (or fewer, under contraction):
          |out - ref| <= |rstd gamma| d0 (1 + rho) + |p| (rho + 2 u) + u |p + beta|,  p = (v - mu) rstd gamma
times 1.001 for the second-order terms, plus 2^-126.  A row scale behind it (gemm_k256) multiplies value and bound and rounds once
more; a scale of 0 leaves an exact 0.  bf16 outputs are held to gemm_cases.bf16_interval(ref, bound).  The CPU test shows that
float32 LayerNorms in three summation orders stay inside the bound and that a LayerNorm without eps, one with the variance over
N - 1 and one with the other stage's gamma / beta fall outside it; the ratios measured on an MI355X stand in test_packed_exact_gpu.py.

FRONT END (FrontCase).  x in {-2 .. 2}, CMVN mean integers, istd in {0.5, 1, 2}, W1 = int_matrix(256, 9, 0.5), b1 / b2 in {-3 .. 3},
W2 = int_matrix(256, 2304, 0.5): act1 is a multiple of 1/2 below 128 (bf16-exact; the head + tail split of the fused kernel has
zero tails), the conv2 sums are multiples of 1/2 below 2^23, so every path must give bf16(relu(.)) of the int64 sums, rounded to
nearest even.
"""
import math

import torch

import gemm_cases as G

U = G.U
D_MODEL = 256
FFN_TILE = (64, 256)       # rows per workgroup x the whole row
K256_TILE = (64, 256)      # gemm_k256: <= 64 rows x one 256-column block (4 waves x 64 columns)
ROWS_TILE = (64, 256)
CONV_TILE = (128, 256)     # conv2_packed / subsample_fused: 128 output positions x 256 channels
FFN_MS = (1, 63, 65, 193)
FFN_HIDDENS = (256, 512, 2048)
QKV_NS = (256, 512, 768, 1024)
K256_MS = (1, 63, 65, 130, 257)
K256_NS = (256, 512, 768, 1024)
ROWS_KS = (64, 128, 192, 256, 448, 4864)
ROWS_MS = (1, 65, 130)
FRONT_TS = (7, 19, 31, 41, 59)
FRONT_BS = (1, 3)
LN_DEPTH = 65
OLD_FFN_X_TOL, OLD_FFN_LN_TOL = 3e-3, 2e-2   # test_conformer_ops_gpu.py::test_ffn_packed


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _choice(values, n, seed):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), (n,), generator=_gen(seed))]


PI = torch.randperm(D_MODEL, generator=_gen(77))  # output column n of the interval case reads hidden unit 256 p + PI[n]


def unit_owner(j):
    """hidden unit -> (wave, block of the wave's sequence = super-block, position in the 32-unit block)."""
    hb = j // 32
    return hb % 4, hb // 4, j % 32


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def balanced_rows(M, seed):
    """(M, 256) float32: row m is +-s_m with 128 entries of each sign -> (x0, sign)."""
    g = _gen(seed)
    sign = torch.empty(M, D_MODEL)
    for m in range(M):
        sign[m] = (torch.randperm(D_MODEL, generator=g) < 128).float() * 2 - 1
    s = _choice((0.5, 1.0, 2.0, 3.0), M, seed + 1)
    return sign * s[:, None], sign


def ln_params_exact(seed):
    """gamma in {1, 2}, |beta| in {3, 4, 5} with either sign: sign * gamma + beta is never 0."""
    return _choice((1.0, 2.0), D_MODEL, seed), _choice((-5.0, -4.0, -3.0, 3.0, 4.0, 5.0), D_MODEL, seed + 1)


def ln64(v, gamma, beta, eps):
    v = v.double()
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ln_bound(v, gamma, beta, eps, depth=LN_DEPTH, row_scale=None):
    """(ref, bound), float64, of the one-pass float32 LayerNorm of the rows v (the module docstring)."""
    v, gamma, beta = v.double(), gamma.double(), beta.double()
    eps = float(torch.tensor(eps, dtype=torch.float32))
    g, g1 = depth * U / (1 - depth * U), (depth + 1) * U / (1 - (depth + 1) * U)
    mu = v.mean(-1, keepdim=True)
    A, E2 = v.abs().mean(-1, keepdim=True), (v * v).mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    dm = g * A
    dsq = (2 * mu.abs() * dm + dm * dm) * (1 + U) + U * mu * mu
    dV = g1 * E2 + dsq
    dV = dV + U * (var + dV)
    T = var + eps
    dT = dV + U * (T + dV)
    assert bool((dT < 0.5 * T).all()), "variance too small for the bound: the case must keep sigma^2 + eps above the summation error"
    rho = (1 - dT / T) ** -0.5 - 1 + 9 * U
    rstd = T ** -0.5
    c = v - mu
    p = c * rstd * gamma
    ref = p + beta
    d0 = dm + U * (c.abs() + dm)
    bound = 1.001 * ((rstd * gamma).abs() * d0 * (1 + rho) + p.abs() * (rho + 2 * U) + U * ref.abs()) + 2.0 ** -126
    if row_scale is not None:
        rs = row_scale.double()[:, None]
        ref, bound = ref * rs, bound * rs.abs() + U * (ref * rs).abs()
    return ref, bound


def _seq_sum(cols):
    """float32 sum of the columns of `cols` (rows, n) in index order, one addition at a time."""
    s = cols[:, 0].clone()
    for i in range(1, cols.shape[1]):
        s = s + cols[:, i]
    return s


def _tree_sum(cols):
    while cols.shape[1] > 1:
        cols = cols[:, 0::2] + cols[:, 1::2]
    return cols[:, 0]


def ln32(v, gamma, beta, eps, order="lanes", use_eps=True, ddof=0):
    """The kernels' one-pass LayerNorm in float32 on the CPU.  order: "lanes" = ffn_packed.hip (lane g sums features 16 j + 4 g + r
    one after the other, then two shuffles), "tree" = pairwise, "k256" = gemm_k256.hip (quads, 4 per lane, shuffles, 4 waves)."""
    v = v.float()
    M = v.shape[0]

    def total(x):
        if order == "lanes":
            lanes = x.view(M, 16, 4, 4).permute(0, 2, 1, 3).reshape(M, 4, 64)
            part = torch.stack([_seq_sum(lanes[:, gq]) for gq in range(4)], 1)
            return (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
        if order == "tree":
            return _tree_sum(x)
        q = x.view(M, 4, 4, 4, 4)                                  # (wave, jt, g, r)
        quad = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])   # (wave, jt, g)
        lane = _seq_sum(quad.permute(0, 1, 3, 2).reshape(M * 16, 4)).view(M, 4, 4)  # (wave, g)
        wave = (lane[:, :, 0] + lane[:, :, 1]) + (lane[:, :, 2] + lane[:, :, 3])
        return (wave[:, 0] + wave[:, 1]) + (wave[:, 2] + wave[:, 3])

    n = v.shape[1]
    mean = (total(v) * (1.0 / n))[:, None]
    q = total(v * v)[:, None] * (1.0 / n)
    var = (q - mean * mean).clamp(min=0)
    if ddof:
        var = var * (n / (n - ddof))
    rstd = 1.0 / torch.sqrt(var + (torch.tensor(eps, dtype=torch.float32) if use_eps else 0.0))
    return (v - mean) * rstd * gamma.float() + beta.float()


def ln32_two_pass(v, gamma, beta, eps):
    """The input LayerNorm of ffn_packed.hip (two passes) in float32."""
    v = v.float()
    mean = _tree_sum(v)[:, None] * (1.0 / 256.0)
    d = v - mean
    var = _tree_sum(d * d)[:, None] * (1.0 / 256.0)
    return d * (1.0 / torch.sqrt(var + eps)) * gamma.float() + beta.float()


# ---- FFN ---------------------------------------------------------------------------------------------------------------------------
def swish_chain32(y, r_ulps=0):
    """The kernels' Swish in float32: t = fl(-log2 e) y, exp2, 1 +, reciprocal (moved by r_ulps ULP), y r."""
    y = y.float()
    t = y * torch.tensor(-1.4426950408889634, dtype=torch.float32)
    r = 1.0 / (1.0 + torch.exp2(t))
    if r_ulps:
        r = (r.view(torch.int32) + r_ulps).view(torch.float32)
    return y * r


class FfnCase:
    """kind "sat" / "act" (the module docstring); ln_in: the activation is LayerNorm(x0; gamma0, beta0) of balanced rows, computed by
    the kernel (a = NULL) - self.a then holds its exact value."""

    def __init__(self, M, hidden, kind="sat", ln_in=False, seed=0, alpha=1.0):
        self.M, self.hidden, self.kind, self.ln_in, self.alpha = M, hidden, kind, ln_in, alpha
        s = seed * 32
        self.gamma0, self.beta0 = ln_params_exact(s + 1)
        if ln_in:
            self.x0, self.sign = balanced_rows(M, s + 3)
            self.a = (self.sign * self.gamma0 + self.beta0).bfloat16()
        else:
            self.x0 = torch.randint(-8, 9, (M, D_MODEL), generator=_gen(s + 3)).float() if kind == "sat" else torch.zeros(M, D_MODEL)
            self.a = (torch.randint(-2, 3, (M, D_MODEL), generator=_gen(s + 4)).bfloat16() if kind == "sat"
                      else G.int_matrix(M, D_MODEL, G.act_density(D_MODEL), s + 4))
        if kind == "sat":
            self.w1 = torch.zeros(hidden, D_MODEL)
            j = torch.arange(hidden)
            mag = torch.randint(1, 3, (hidden, 8), generator=_gen(s + 5)) * (torch.randint(0, 2, (hidden, 8), generator=_gen(s + 6)) * 2 - 1)
            for ks in range(8):
                self.w1[j, 32 * ks + (j + 5 * ks) % 32] = mag[:, ks].float()
            self.w1 = self.w1.bfloat16()
            self.b1 = (132.0 if ln_in else 64.0) + G.int_vector(hidden, -3, 3, s + 7)
            self.w2 = G.int_matrix(D_MODEL, hidden, 0.5, s + 8)
            self.b2 = G.int_vector(D_MODEL, -3, 3, s + 9)
        else:
            # (LayerNorm rows are dense with |a| <= 7: a sparser W1 keeps the pre-activations in the range where Swish bends)
            self.w1 = G.int_matrix(hidden, D_MODEL, 0.01 if ln_in else G.act_density(D_MODEL), s + 5)
            self.b1 = G.int_vector(hidden, -3, 3, s + 7)
            self.w2, self.b2, self.alpha = None, torch.zeros(D_MODEL), 1.0

    def passes(self):
        return self.hidden // D_MODEL if self.kind == "act" else 1

    def w2_pass(self, p):
        if self.kind == "sat":
            return self.w2
        w = torch.zeros(D_MODEL, self.hidden)
        w[torch.arange(D_MODEL), D_MODEL * p + PI] = 1
        return w.bfloat16()

    def y(self):
        """The exact pre-activations (float64)."""
        return self.a.double() @ self.w1.double().T + self.b1.double()

    def x_ref(self, p=0):
        """kind "sat": the exact x (float64).  kind "act": (lo, hi) float32 of pass p."""
        if self.kind == "sat":
            y = self.y()
            assert float(y.min()) >= 16 and float(y.max()) <= 255
            return self.x0.double() + self.alpha * (y @ self.w2.double().T + self.b2.double())
        y = self.y()[:, D_MODEL * p + PI]
        lo, hi = G.bf16_interval(G.act64(y, G.ACT_SWISH), G.act_bound(y, G.ACT_SWISH))
        return self.x0 + lo.float(), self.x0 + hi.float()

    def explain(self, p=0):
        def f(r, c, got):
            j = D_MODEL * p + int(PI[c])
            return "hidden unit %d = (wave %d, block %d of the wave, position %d), y = %g" % ((j,) + unit_owner(j) + (float(self.y()[r, j]),))
        return f


def ffn_model(a, w1, b1, w2, b2, x0, alpha, defect=None, units=()):
    """float64 model of one launch on any (a, W1, b1, W2, b2, x0), with one planted defect; h is rounded to bf16 as the kernels do.
    defects: trunc_h, no_b1 (units), drop_last_kstep (units), exp_const, drop_unit (units), swap_b1, drop_o_block (one block of 32
    units of the second product, units[0] names it), b2_unscaled, tile_twice (rows 64 .. 127 updated twice)."""
    u = list(units)
    y = a.double() @ w1.double().T
    if defect == "drop_last_kstep":
        y[:, u] -= a[:, 224:].double() @ w1[u, 224:].double().T
    bb = b1.double().clone()
    if defect == "swap_b1":
        bb = bb.view(-1, 2, 4).flip(1).reshape(-1)
    if defect == "no_b1":
        bb[u] = 0
    y = y + bb
    h = y * torch.sigmoid(y * (1.002 if defect == "exp_const" else 1.0))
    h = (G.truncate_bf16(h.float()) if defect == "trunc_h" else h.float().bfloat16()).double()
    if defect == "drop_unit":
        h[:, u] = 0
    if defect == "drop_o_block":
        blk = u[0] // 32
        h[:, 32 * blk:32 * blk + 32] = 0
    o = h @ w2.double().T
    upd = alpha * o + (1.0 if defect == "b2_unscaled" else alpha) * b2.double()
    x = x0.double() + upd
    if defect == "tile_twice":
        x[64:128] += upd[64:128]
    return x


def old_ffn_case():
    """test_conformer_ops_gpu.py::test_ffn_packed at (250, 2048): its random operands, restated."""
    def rand(*shape, seed, scale=1.0):
        return torch.randn(*shape, generator=_gen(seed)) * scale
    m, hidden, d = 250, 2048, 256
    return dict(a=rand(m, d, seed=90).bfloat16(), w1=rand(hidden, d, seed=91, scale=1.0 / 16).bfloat16(), b1=rand(hidden, seed=92, scale=0.3),
                w2=rand(d, hidden, seed=93, scale=1.0 / math.sqrt(hidden)).bfloat16(), b2=rand(d, seed=94, scale=0.3),
                x0=rand(m, d, seed=95) * 3 + 0.5, alpha=0.5, g1=1 + 0.1 * rand(d, seed=96), be1=0.1 * rand(d, seed=97))


def old_ffn_check(x, xs, g1, be1):
    """The two whole-tensor checks of test_ffn_packed (ln_mode 1) on a model output x against the float64 chain xs."""
    ok_x = float((x - xs).abs().max()) <= OLD_FFN_X_TOL * float(xs.abs().max())
    ok_ln = float((ln64(x, g1, be1, 1e-5) - ln64(xs, g1, be1, 1e-5)).abs().max()) <= OLD_FFN_LN_TOL
    return ok_x, ok_ln


class QkvCase:
    """The tail of ma_ffn_packed_qkv_bf16 with W2 = 0, b2 = 0: x stays the balanced x0 and LN(x) gamma1 + beta1 is exact, so
    qkv_out = bf16(a1 Wq^T + bias) of integers.  Hot rows of Wq are all 2 with an odd bias; every fourth column has a bias of k + 1/2:
    sums of magnitude 128 .. 255 (bf16 step 1) are then exactly halfway."""

    def __init__(self, M, N, hidden=256, seed=0):
        s = seed * 32
        self.M, self.N, self.hidden = M, N, hidden
        self.x0, self.sign = balanced_rows(M, s + 1)
        self.gamma1, self.beta1 = ln_params_exact(s + 3)
        self.a1 = self.sign * self.gamma1 + self.beta1
        self.wq = G.int_matrix(N, D_MODEL, 0.5, s + 5)
        self.hot = G.hot_indices(N)
        self.wq[self.hot] = 2
        self.bias = G.int_vector(N, -3, 3, s + 6)
        self.bias[::4] += 0.5
        self.bias[self.hot] = 1.0
        c = FfnCase(M, hidden, "sat", seed=seed + 7)
        self.a, self.w1, self.b1 = c.a, c.w1, c.b1          # a live first product whose result W2 = 0 discards
        self.w2, self.b2 = torch.zeros(D_MODEL, hidden, dtype=torch.bfloat16), torch.zeros(D_MODEL)

    def ref(self):
        return self.a1.double() @ self.wq.double().T + self.bias.double()

    def explain(self, r, c, got):
        return "output column %d = (wave %d, column block %d of the wave, position %d)" % ((c,) + unit_owner(c))


def tie_stats(ref):
    """(share of exact ties, ties below an even neighbour, below an odd one) of the float32 values ref about to be rounded to bf16."""
    f = ref.float().contiguous()
    tie = G.is_tie(f)
    odd = ((f.view(torch.int32) >> 16) & 1) == 1   # the truncated bf16 is odd: round-to-even goes up
    return float(tie.float().mean()), int((tie & ~odd).sum()), int((tie & odd).sum())


# ---- gemm_k256 / rows_packed ---------------------------------------------------------------------------------------------------------
class DenseCase(G.Case):
    """gemm_cases.Case with ties in the bulk of a K = 256 product as well: its sums have a standard deviation of 20, where bf16 still
    holds every integer, so every fourth column (never a hot one) gets a bias of k + 1/16 - exactly halfway wherever 16 <= |v| < 32.
    Everything stays a multiple of 1/32 (alpha 0.5) far below 2^23 / 32."""

    def __init__(self, M, N, K, **kw):
        super().__init__(M, N, K, **kw)
        cols = [n for n in range(1, N, 4) if n not in self.hot_cols]
        self.bias[cols] += 1.0 / 16


def explain_fragment(M, N, K):
    def f(r, c, got):
        k0 = G.hot_k(r, K)
        return G.explain_address(r, c, got, M, N, K) + "; the wanted element sits in k-step %d, lane group %d, column tile %d" % (
            k0 // 32, (k0 % 32) // 8, c // 16)
    return f


# ---- front end -----------------------------------------------------------------------------------------------------------------------
class FrontCase:
    def __init__(self, B, T, idim=80, C=256, cmvn=True, seed=0):
        s = seed * 32
        self.B, self.T, self.idim, self.C, self.cmvn = B, T, idim, C, cmvn
        self.x = torch.randint(-2, 3, (B, T, idim), generator=_gen(s + 1)).float()
        self.mean = G.int_vector(idim, -2, 2, s + 2)
        self.istd = _choice((0.5, 1.0, 2.0), idim, s + 3)
        self.w1 = G.int_matrix(256, 9, 0.5, s + 4).float()[:C].contiguous()
        self.b1 = G.int_vector(256, -3, 3, s + 5)[:C].contiguous()
        self.w2 = G.int_matrix(256, 2304, 0.5, s + 6).view(256, 3, 3, 256)   # (Cout, kh, kw, C)
        self.b2 = G.int_vector(256, -3, 3, s + 7)
        self.T1, self.F1 = (T - 3) // 2 + 1, (idim - 3) // 2 + 1
        self.T2, self.F2 = (self.T1 - 3) // 2 + 1, (self.F1 - 3) // 2 + 1
        self._act1 = self._cols = None

    def act1(self):
        """(B, T1, F1, C) float64, exact."""
        if self._act1 is None:
            xin = ((self.x - self.mean) * self.istd if self.cmvn else self.x).double()
            y = torch.nn.functional.conv2d(xin[:, None], self.w1.double().view(self.C, 1, 3, 3), self.b1.double(), stride=2)
            self._act1 = y.clamp(min=0).permute(0, 2, 3, 1).contiguous()
        return self._act1

    def columns(self, seam_defect=None):
        """im2col of act1 for conv2: (B T2 F2, 9 C), k = (kh, kw, c).  seam_defect = (position, tap): that tap of that output position
        reads the patch one feature position to the right."""
        a = self.act1()
        a = torch.nn.functional.pad(a, (0, 0, 0, 1))  # (one spare feature column for the defect)
        cols = [a[:, kh:kh + 2 * self.T2 - 1:2, kw:kw + 2 * self.F2 - 1:2, :] for kh in range(3) for kw in range(3)]
        out = torch.cat(cols, dim=-1).reshape(self.B * self.T2 * self.F2, 9 * self.C).clone()
        if seam_defect is not None:
            pos, tap = seam_defect
            b, rem = divmod(pos, self.T2 * self.F2)
            t2, f2 = divmod(rem, self.F2)
            kh, kw = divmod(tap, 3)
            out[pos, tap * self.C:(tap + 1) * self.C] = a[b, 2 * t2 + kh, 2 * f2 + kw + 1]
        return out

    def z2(self, seam_defect=None):
        """The conv2 sums + b2 before the ReLU (float64, exact), (B T2 F2, 256)."""
        return self.columns(seam_defect) @ self.w2.reshape(256, -1).double().T + self.b2.double()

    def out(self, seam_defect=None):
        return self.z2(seam_defect).clamp(min=0)

    def explain(self, r, c, got):
        """Flat output row r -> utterance, its 128-position tile, the position in the tile and the output (row, column) of the map."""
        b, rem = divmod(r, self.T2 * self.F2)
        return "utterance %d, tile %d of the utterance, position %d in the tile = output (t %d, f %d); channel %d = consumer wave %d" % (
            b, rem // 128, rem % 128, rem // self.F2, rem % self.F2, c, c // 64)


class SplitCase(FrontCase):
    """subsample_fused computes a float32 product of conv1 as xh wh + xh wl + xl wh on bf16 heads and tails.  x = I + J 2^-10,
    W1 = P + Q 2^-10 with I, P in {-2, -1, 1, 2} and J, Q in {-2 .. 2}: the heads are I and P, the tails J 2^-10 and Q 2^-10 (all exact
    bf16 values), and the nine-tap sum of the three terms is a multiple of 2^-10 below 64 - exact in float32 in any order.  The
    reference is that sum (WITHOUT xl wl).  b1 is 0 on the even channels and an integer on the odd ones: where the heads cancel, act1 is
    the tail sum alone, a bf16-exact multiple of 2^-10.  W2 of pass p is one-hot - output channel n reads act1 channel n at tap p - and
    b2 = 0, so out == bf16(act1) gathered at patch position (2 t + kh, 2 f + kw)."""

    def __init__(self, B, T, seed=0):
        super().__init__(B, T, cmvn=False, seed=seed)
        s = seed * 32 + 16

        def nz(shape, sd):
            return torch.randint(1, 3, shape, generator=_gen(sd)).float() * (torch.randint(0, 2, shape, generator=_gen(sd + 1)) * 2 - 1).float()
        self.xh, self.xl = nz((B, T, 80), s), torch.randint(-2, 3, (B, T, 80), generator=_gen(s + 2)).float() * 2.0 ** -10
        self.wh, self.wl = nz((256, 9), s + 3), torch.randint(-2, 3, (256, 9), generator=_gen(s + 5)).float() * 2.0 ** -10
        self.x, self.w1 = self.xh + self.xl, self.wh + self.wl
        self.b1 = G.int_vector(256, -3, 3, s + 6)
        self.b1[0::2] = 0
        self.b2 = torch.zeros(256)

    def _conv(self, x, w):
        return torch.nn.functional.conv2d(x.double()[:, None], w.double().view(256, 1, 3, 3), stride=2).permute(0, 2, 3, 1)

    def act1(self, drop=None):
        """bf16(relu(b1 + xh wh + xh wl + xl wh)) as float64, (B, T1, F1, 256); drop = "xh_wl" / "xl_wh" leaves that term out."""
        z = self._conv(self.xh, self.wh) + self.b1.double()
        if drop != "xh_wl":
            z = z + self._conv(self.xh, self.wl)
        if drop != "xl_wh":
            z = z + self._conv(self.xl, self.wh)
        return z.clamp(min=0).float().bfloat16().double()

    def w2_pass(self, p):
        w = torch.zeros(256, 9, 256)
        w[torch.arange(256), p, torch.arange(256)] = 1
        return w.view(256, 3, 3, 256).bfloat16()

    def out_pass(self, p, drop=None):
        kh, kw = divmod(p, 3)
        a = self.act1(drop)
        return a[:, kh:kh + 2 * self.T2 - 1:2, kw:kw + 2 * self.F2 - 1:2, :].reshape(-1, 256)

    def explain_pass(self, p):
        def f(r, c, got):
            b, rem = divmod(r, self.T2 * self.F2)
            t2, f2 = divmod(rem, self.F2)
            kh, kw = divmod(p, 3)
            return "tap %d = (kh %d, kw %d), act1 patch position (t %d, f %d) of utterance %d, channel %d = chunk %d; %s" % (
                p, kh, kw, 2 * t2 + kh, 2 * f2 + kw, b, c, c // 32, FrontCase.explain(self, r, c, got))
        return f
