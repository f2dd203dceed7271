"""Inputs, references and comparators of the GEMM tests (test_gemm_cases_cpu.py, test_gemm_exact_gpu.py): ma_gemm_bf16,
ma_conv1d_taps_bf16, ma_conv2d_3x3s2_nhwc_bf16 and ma_gemm_bf16_splitk_f32 of csrc/gemm_bf16.hip.  Nothing here needs a device; every
function works on whatever device its tensors live on (the GPU test evaluates the float64 references there).

EXACT CASES.  A and W hold integers of {-2 .. 2} (a fixed share of them non-zero), bias / residual / col_scale / col_shift small integers
in float32, row_scale in {0, 1, 2}, alpha in {1, 0.5, 2}.  Every partial sum of the contraction and every intermediate of the epilogue
is then an integer multiple of 1/2 of magnitude below 2^23 (exact_bound() states the worst case; the CPU test checks it per case): the
float32 result does not depend on the accumulation order or on FMA contraction and EQUALS an int64 / float64 evaluation.  A float32
output must equal the reference, a bf16 output must equal ref.float().bfloat16() (round to nearest even of an exact float32).  A few
"hot" rows of A and columns of W are all 2: their products are 4 K >= 256, and the bias of the hot columns puts them exactly halfway
between two bf16 numbers, once below an even and once below an odd neighbour, so truncation and round-half-up both fail.
(+0 and -0 compare equal: the sign of a zero product depends on the order in which the zero factors are applied.)

ADDRESS CASES.  Row m of A is one-hot at k = hot_k(m), W[n, k] = ((31 n + 17 k) mod 251) - 125: out[m, n] = W[n, hot_k(m)], and
explain_address() names the (m, n, k) a wrong element came from.

GUARD BANDS.  Window puts the M x N output at [top : top + M, off : off + N] of a larger buffer filled with a canary bit pattern (a
NaN for float32, another NaN pattern for bf16).  check_window() wants every bit outside the window unchanged and reports the first wrong
(row, column) inside it with its tile and its position in the tile.

NON-EXACT ACTIVATIONS (swish, sigmoid, tanh; float32 output).  The pre-activation y is an exact integer, the reference is float64 on y.
apply_act (gemm_bf16.hip) computes, with u = 2^-24 (one float32 rounding) and the accuracy the CDNA instruction-set guide states for
v_exp_f32 and v_rcp_f32 (1 ULP = 2 u relative):
    t = c * y            c = fl(-log2 e) (relative error u), one rounding: t = -y log2(e) (1 + d), |d| <= 2 u
    e = exp2(t)          the argument error is a relative error ln 2 * |t| * 2 u = 2 u |y| of the result, plus 2 u of the instruction
    d = 1 + e            one rounding; the error of e enters with weight e / (1 + e) = 1 - sigmoid(y) =: w
    r = rcp(d)           2 u
  sigmoid = r:           relative error <= u (2 (|y| + 1) w + 3)                                          =: rho(y)
  swish = y * r:         one more rounding: relative error <= rho(y) + u
  tanh = 2 r - 1, r = sigmoid(2 y): 2 r is exact; for y >= 0 the subtraction is exact (2 r in [1, 2]), for y < 0 it rounds once at a
                         result of magnitude <= 1.  ABSOLUTE error <= 2 sigmoid(2 y) rho(2 y) + u: at y = 0 that is 5 u against a result of
                         0 - the cancellation leaves no relative bound, hence the absolute term.
Terms of second order in u are covered by the factor 1.001; exp2 overflowing to inf (y <= -89) gives r = 0 against a true value below
2^-126, and results below 2^-126 may be flushed: an absolute 2^-126 (1 + |y|) is added.  What follows the activation in these cases
(row_scale, alpha) is an exact scaling of value and bound.  bf16 outputs: the device rounds a float32 v with |v - ref| <= bound to
nearest even; rounding is monotone, so the output lies in [bf16(ref - bound), bf16(ref + bound)], never more than one bf16 step from
bf16(ref).  The errors measured on an MI355X stand in the docstring of test_gemm_exact_gpu.py.
"""
import math

import torch

ACT_NONE, ACT_SWISH, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4
U = 2.0 ** -24
F32_CANARY = 0x7FC0BEEF   # a quiet NaN
BF16_CANARY = 0x7FA5      # another NaN pattern
OLD_F32_TOL = 2e-5        # test_conformer_ops_gpu.py: max |got - ref| <= 2e-5 max |ref|, over the whole tensor
OLD_BF16_TOL = 2.0 ** -8 * 1.01

# kernel name -> (tile rows, tile columns): how check_window names the position of a wrong element
TILES = {"ws512": (32, 128), "8ph": (256, 256), "t128": (128, 128), "t64": (64, 128)}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def int_matrix(rows, cols, density, seed):
    """(rows, cols) bf16 on the CPU: a share `density` of the entries uniform in {-2, -1, 1, 2}, the rest 0."""
    g = _gen(seed)
    mag = torch.randint(1, 3, (rows, cols), generator=g)
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    keep = torch.rand(rows, cols, generator=g) < density
    return (mag * sign * keep).to(torch.bfloat16)


def int_vector(n, lo, hi, seed):
    return torch.randint(lo, hi + 1, (n,), generator=_gen(seed)).float()


def act_density(K):
    """The share of non-zero entries at which the pre-activations have a variance of 20 (K (2.5 d)^2): two thirds within |z| <= 4."""
    return min(0.5, math.sqrt(20.0 / K) / 2.5)


def bf16_step(x):
    """One bf16 step (8 significant bits) at |x| (x float64 tensor or float), 0 at 0."""
    x = torch.as_tensor(x, dtype=torch.float64).abs()
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp(min=2.0 ** -126))) - 7), torch.zeros_like(x))


def is_tie(x):
    """float tensor of exact float32 values -> bool: exactly halfway between two bf16 numbers."""
    return (x.float().contiguous().view(torch.int32) & 0xFFFF) == 0x8000


HOT_ROWS_FRAC = (0.0, 0.37, 1.0)  # first row, one inside, the last row (of the ragged last tile)


def hot_indices(n, count=3):
    return sorted({min(n - 1, int(f * (n - 1))) for f in HOT_ROWS_FRAC[:count]})


class Case:
    """One product: A (M, K) and W (N, K) with their epilogue vectors, all on the CPU until .to(device)."""

    def __init__(self, M, N, K, density=0.5, seed=0, hot=True, tag=""):
        self.M, self.N, self.K, self.density, self.tag = M, N, K, density, tag
        self.a = int_matrix(M, K, density, seed * 16 + 1)
        self.w = int_matrix(N, K, density, seed * 16 + 2)
        self.bias = int_vector(N, -3, 3, seed * 16 + 3)
        self.hot_rows, self.hot_cols = [], []
        if hot:
            self.hot_rows, self.hot_cols = hot_indices(M), hot_indices(N)
            self.a[self.hot_rows] = 2
            self.w[self.hot_cols] = 2
            step = float(bf16_step(4.0 * K))
            assert step >= 2 and (4 * K) % int(step) == 0
            for i, n in enumerate(self.hot_cols):  # 4 K + step / 2 and 4 K + 3 step / 2: ties below an even and an odd neighbour
                self.bias[n] = (step / 2) * (1 + 2 * ((i + (4 * K // int(step))) % 2))
        self.col_scale = int_vector(N, 1, 3, seed * 16 + 4) * (torch.randint(0, 2, (N,), generator=_gen(seed * 16 + 5)) * 2 - 1).float()
        self.col_shift = int_vector(N, -3, 3, seed * 16 + 6)
        self.row_scale = int_vector(M, 0, 2, seed * 16 + 7)
        self.residual = torch.randint(-8, 9, (M, N), generator=_gen(seed * 16 + 8)).float()
        self._z = None

    def to(self, device):
        for k in ("a", "w", "bias", "col_scale", "col_shift", "row_scale", "residual"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def z(self):
        """A . W^T in float64 (exact: integers far below 2^53), computed once."""
        if self._z is None:
            self._z = self.a.double() @ self.w.double().T
        return self._z


def z_int64(a, w):
    return a.long() @ w.long().T


def exact_bound(K, taps_or_one=1):
    """The largest magnitude any intermediate of an exact case can take: (4 K + |bias|) * |col_scale| + |col_shift|, times row_scale 2
    and alpha 2, plus |residual|; hot columns carry a bias of up to 3/2 bf16 steps of 4 K (4 K / 128 * 1.5)."""
    kk = K * taps_or_one
    return ((4 * kk + max(3, 4 * kk * 1.5 / 128)) * 3 + 3) * 4 + 8


# ---- epilogues -----------------------------------------------------------------------------------------------------------------------
# name -> dict(bias, act, affine, act2, row_scale, alpha, residual): which terms of ma_gemm_epilogue_t the launch sets
EPILOGUES = {
    "none": dict(),
    "bias": dict(bias=True),
    "bias_rs": dict(bias=True, row_scale=True),
    "bias_relu": dict(bias=True, act=ACT_RELU),
    "bias_rs_half_res": dict(bias=True, row_scale=True, alpha=0.5, residual=True),
    "epi1_affine": dict(bias=True, act=ACT_RELU, affine=True, row_scale=True),            # EPI = 1, exact
    "epi1_chain_tanh": dict(bias=True, act=ACT_RELU, affine=True, act2=ACT_TANH, row_scale=True),  # the ECAPA chain
    "sigmoid": dict(bias=True, act=ACT_SIGMOID),
    "swish": dict(bias=True, act=ACT_SWISH),
    "tanh": dict(bias=True, act=ACT_TANH),
}
NON_EXACT = ("epi1_chain_tanh", "sigmoid", "swish", "tanh")


def act64(v, act):
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def _rho(y):
    w = 1.0 - torch.sigmoid(y)
    return U * (2.0 * (y.abs() + 1.0) * w + 3.0)


def act_bound(y, act):
    """Absolute error bound (float64 tensor) of apply_act(y, act) in float32 for an exact pre-activation y: the module docstring."""
    tiny = 2.0 ** -126 * (1.0 + y.abs())
    if act == ACT_SIGMOID:
        b = torch.sigmoid(y) * _rho(y)
    elif act == ACT_SWISH:
        b = (y * torch.sigmoid(y)).abs() * (_rho(y) + U)
    elif act == ACT_TANH:
        b = 2.0 * torch.sigmoid(2.0 * y) * _rho(2.0 * y) + U
    else:
        return torch.zeros_like(y)
    return 1.001 * b + tiny


def epilogue_ref(z, c, name, residual=None):
    """float64 reference of epilogue `name` on the exact product z (float64) of case c -> (ref, bound): bound is None for an exact
    epilogue, else the per-element absolute bound of a float32 output."""
    e = EPILOGUES[name]
    v = z + c.bias.double() if e.get("bias") else z.clone()
    bound = None
    act, act2 = e.get("act", 0), e.get("act2", 0)
    if act in (ACT_SWISH, ACT_SIGMOID, ACT_TANH):
        bound = act_bound(v, act)
    v = act64(v, act)
    if e.get("affine"):
        assert bound is None
        v = v * c.col_scale.double() + c.col_shift.double()
    if act2:
        assert bound is None and act2 == ACT_TANH
        bound = act_bound(v, act2)
        v = act64(v, act2)
    scale = torch.full((z.shape[0], 1), float(e.get("alpha", 1.0)), dtype=torch.float64, device=z.device)
    if e.get("row_scale"):
        scale = scale * c.row_scale.double()[:, None]
    v = v * scale
    if bound is not None:
        bound = bound * scale
    if e.get("residual"):
        v = v + (c.residual if residual is None else residual).double()
    return v, bound


def small_z_share(c, name, rows=256):
    """Share of pre-activations with |y| <= 4 in front of the non-exact activation of epilogue `name`, on a sample of rows."""
    e = EPILOGUES[name]
    idx = torch.arange(0, c.M, max(1, c.M // rows))
    y = c.a[idx].double() @ c.w.double().T + c.bias.double()
    if e.get("act2"):
        y = act64(y, e["act"]) * c.col_scale.double() + c.col_shift.double()
    return float((y.abs() <= 4).double().mean())


# ---- address cases -------------------------------------------------------------------------------------------------------------------
def hot_k(m, K):
    return (7 * m + 3) % K


def address_w(n, k):
    return ((31 * n + 17 * k) % 251) - 125


def address_case(M, N, K):
    a = torch.zeros(M, K, dtype=torch.bfloat16)
    m = torch.arange(M)
    a[m, hot_k(m, K)] = 1
    w = address_w(torch.arange(N)[:, None], torch.arange(K)[None, :]).to(torch.bfloat16)
    want = address_w(torch.arange(N)[None, :], hot_k(m, K)[:, None]).float()
    return a, w, want


def explain_address(m, n, got, M, N, K):
    """Where a wrong value of an address case can have come from: the k of row n that hold it, and the rows / columns whose own
    element it is."""
    k0 = hot_k(m, K)
    ks = [k for k in range(K) if address_w(n, k) == got][:4]
    ns = [n2 for n2 in range(max(0, n - 256), min(N, n + 257)) if address_w(n2, k0) == got][:4]
    ms = [m2 for m2 in range(max(0, m - 256), min(M, m + 257)) if address_w(n, hot_k(m2, K)) == got][:4]
    return "want W[n=%d, k=%d] = %d of row m=%d; got %s = W[n, k in %s] = W[n in %s, k] = element of rows %s" % (
        n, k0, address_w(n, k0), m, got, ks, ns, ms)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
LD_KINDS = ("a8", "a8o4", "a4", "odd")


def ld_off(N, kind):
    """(leading dimension, column offset of the window) of layout `kind`: a8 = ld % 8 == 0 and a 16-byte aligned base, a8o4 = the
    window 4 elements further right, a4 = ld % 4 == 0 only, odd = an odd ld, tight = ld == N (guard rows only, for the entry points
    without a leading dimension), pad8 = the window at column 0 of rows of N + 8 elements (convmodule_cases).  Offsets are multiples of
    4 elements."""
    ld8 = (N + 16 + 7) // 8 * 8
    return {"a8": (ld8, 8), "a8o4": (ld8, 4), "a4": (ld8 + 4, 4), "odd": (ld8 + 3, 4), "tight": (N, 0), "pad8": (N + 8, 0)}[kind]


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


class Window:
    """An (M, N) output window inside a canary-filled buffer with `top` rows above, `bottom` rows below and columns on both sides."""

    def __init__(self, M, N, dtype, kind="a8", device="cpu", top=2, bottom=3):
        self.M, self.N, self.top = M, N, top
        self.ld, self.off = ld_off(N, kind)
        self.buf = torch.empty(top + M + bottom, self.ld, dtype=dtype, device=device)
        _bits(self.buf).fill_(F32_CANARY if dtype == torch.float32 else BF16_CANARY)
        self.view = self.buf[top:top + M, self.off:self.off + N]
        self.before = None

    def snapshot(self):
        """Call after any prefill of the window (the in-place residual) and before the launch."""
        self.before = _bits(self.buf).clone()
        return self


def check_window(win, want, tile=(64, 128), bound=None, lo=None, hi=None, explain=None):
    """None if the buffer of `win` is right after a launch, else a message.  Outside the window every bit must be what snapshot() saw.
    Inside: got == want (exact cases; want in the buffer's dtype), or |got - want| <= bound per element (float64 want and bound), or
    lo <= got <= hi (bf16 outputs of the non-exact activations)."""
    M, N, top, off = win.M, win.N, win.top, win.off
    changed = _bits(win.buf) != win.before
    changed[top:top + M, off:off + N] = False
    if bool(changed.any()):
        r, c = [int(x) for x in changed.nonzero()[0]]
        return "guard band overwritten at buffer row %d (window row %d of %d), column %d (window column %d of %d): bits %#x" % (
            r, r - top, M, c, c - off, N, int(_bits(win.buf)[r, c]) & 0xFFFFFFFF)
    got = win.view
    if lo is not None:
        bad = ~((got.double() >= lo.double()) & (got.double() <= hi.double()))
    elif bound is not None:
        bad = ~((got.double() - want).abs() <= bound)
    else:
        assert want.dtype == got.dtype and want.shape == got.shape
        bad = ~(got == want)
    if not bool(bad.any()):
        return None
    r, c = [int(x) for x in bad.nonzero()[0]]
    msg = "%d wrong elements, first at (row %d, column %d): tile (%d, %d), position (%d, %d) in the tile; got %r want %r" % (
        int(bad.sum()), r, c, r // tile[0], c // tile[1], r % tile[0], c % tile[1], float(got[r, c]),
        float(want[r, c]) if want is not None else (float(lo[r, c]), float(hi[r, c])))
    if bound is not None:
        msg += " bound %.3e" % float(bound[r, c])
    if explain is not None:
        msg += "; " + explain(r, c, float(got[r, c]))
    return msg


def bf16_interval(ref, bound):
    """[bf16(ref - bound), bf16(ref + bound)] (the bound widened by one float32 rounding of the float64 -> float32 conversion)."""
    b = bound + ref.abs() * 2.0 ** -23
    return (ref - b).float().bfloat16(), (ref + b).float().bfloat16()


def old_check_f32(got, ref):
    """The whole-tensor check of test_conformer_ops_gpu.py on an (M, N) float32 output."""
    return float((got.double() - ref.double()).abs().max()) <= OLD_F32_TOL * float(ref.abs().max())


def old_check_bf16(got, ref):
    return float((got.double() - ref.double()).abs().max()) <= OLD_BF16_TOL * float(ref.abs().max())


def truncate_bf16(x):
    """float32 -> bf16 by dropping the low 16 bits (the defect a correct kernel must not have)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ---- Conv1d taps ---------------------------------------------------------------------------------------------------------------------
class TapCase:
    """act buffer (margin + rows + margin, C), W (N, taps, C); the entry point is handed row `margin` of the buffer."""

    def __init__(self, rows, C, taps, dil, N, seed=0, density=0.5, extra_margin=0):
        self.rows, self.C, self.taps, self.dil, self.N = rows, C, taps, dil, N
        self.halo = (taps // 2) * dil
        self.margin = self.halo + extra_margin
        self.K = taps * C
        self.buf = int_matrix(rows + 2 * self.margin, C, density, seed * 16 + 1)  # margins are NOT zero: a row read one off shows
        self.w = int_matrix(N, taps * C, density, seed * 16 + 2).view(N, taps, C)
        self.bias = int_vector(N, -3, 3, seed * 16 + 3)
        hot_r, self.hot_cols = hot_indices(rows), hot_indices(N)
        for r in hot_r:  # every row a tap of a hot output row reads
            for j in range(taps):
                self.buf[self.margin + r + (j - taps // 2) * dil] = 2
        self.w[self.hot_cols] = 2
        step = float(bf16_step(4.0 * self.K))
        for i, n in enumerate(self.hot_cols):
            self.bias[n] = (step / 2) * (1 + 2 * (i % 2))
        self.col_scale = int_vector(N, 1, 3, seed * 16 + 4)
        self.col_shift = int_vector(N, -3, 3, seed * 16 + 6)
        self.row_scale = int_vector(rows, 1, 2, seed * 16 + 7)
        self.row_scale[:self.halo] = 0  # the halo rows of the output are zeroed
        self.row_scale[rows - self.halo:] = 0
        self.M, self.residual = rows, None
        self._z = None

    def to(self, device):
        for k in ("buf", "w", "bias", "col_scale", "col_shift", "row_scale"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def columns(self, off_by_one_tap=None):
        """The im2col matrix (rows, taps * C): column block j is the activation shifted by (j - taps / 2) * dil rows."""
        cols = []
        for j in range(self.taps):
            s = self.margin + (j - self.taps // 2) * self.dil + (1 if off_by_one_tap == j else 0)
            cols.append(self.buf[s:s + self.rows])
        return torch.cat(cols, dim=1)

    def z(self):
        if self._z is None:
            self._z = self.columns().double() @ self.w.reshape(self.N, -1).double().T
        return self._z

    def z_int64(self, off_by_one_tap=None):
        return self.columns(off_by_one_tap).long() @ self.w.reshape(self.N, -1).long().T

    def z_conv1d(self):
        x = self.buf.double().T[None]  # (1, C, rows + 2 margin)
        y = torch.nn.functional.conv1d(x, self.w.double().permute(0, 2, 1), dilation=self.dil)[0].T  # valid positions
        s = self.margin - self.halo
        return y[s:s + self.rows]


# ---- Conv2d 3x3 stride 2 -------------------------------------------------------------------------------------------------------------
class Conv2dCase:
    def __init__(self, B, H, Wd, C, Cout, seed=0, density=0.5):
        self.B, self.H, self.Wd, self.C, self.Cout = B, H, Wd, C, Cout
        self.Ho, self.Wo = (H - 3) // 2 + 1, (Wd - 3) // 2 + 1
        self.M, self.N, self.K = B * self.Ho * self.Wo, Cout, 9 * C
        self.act = int_matrix(B * H * Wd, C, density, seed * 16 + 1).view(B, H, Wd, C)
        self.w = int_matrix(Cout, 9 * C, density, seed * 16 + 2).view(Cout, 3, 3, C)
        self.bias = int_vector(Cout, -3, 3, seed * 16 + 3)
        self.hot_cols = hot_indices(Cout)
        self.act[0, :3, :3] = 2  # output position (0, 0, 0) is hot
        self.w[self.hot_cols] = 2
        step = float(bf16_step(4.0 * self.K))
        for i, n in enumerate(self.hot_cols):
            self.bias[n] = (step / 2) * (1 + 2 * (i % 2))
        self._z = None

    def to(self, device):
        for k in ("act", "w", "bias"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def columns(self):
        cols = [self.act[:, kh:kh + 2 * self.Ho - 1:2, kw:kw + 2 * self.Wo - 1:2, :] for kh in range(3) for kw in range(3)]
        return torch.cat(cols, dim=-1).reshape(self.M, self.K)

    def z(self):
        if self._z is None:
            self._z = self.columns().double() @ self.w.reshape(self.Cout, -1).double().T
        return self._z

    def z_conv2d(self):
        y = torch.nn.functional.conv2d(self.act.double().permute(0, 3, 1, 2), self.w.double().permute(0, 3, 1, 2), stride=2)
        return y.permute(0, 2, 3, 1).reshape(self.M, self.Cout)


# ---- planted defects (CPU test): each returns what a kernel with that defect would leave in the window's buffer -----------------------
def tile_permutation_defect(ntiles, twice, never):
    """The bid -> tile map of an 8-phase launch whose tile order is no bijection: `twice` is computed by two workgroups, `never` by none."""
    perm = list(range(ntiles))
    perm[never] = twice
    return perm


# ---- the cases of test_gemm_exact_gpu.py (shapes for the 256 CUs of an MI355X) ---------------------------------------------------------
# kernel codes of ma_gemm_bf16_variant (MA_GEMM_KERNEL_*)
WS512, G8_ROW, G8_BLK, T128X2, T64X2, T64X3 = 1, 2, 3, 4, 5, 6
KERNEL_TILE = {WS512: TILES["ws512"], G8_ROW: TILES["8ph"], G8_BLK: TILES["8ph"], T128X2: TILES["t128"], T64X2: TILES["t64"],
               T64X3: TILES["t64"]}
# id -> (kernel, M, N, K): every M leaves a ragged last row tile, every N but the weight-stationary ones a ragged last column tile with N % 4 != 0
KERNEL_SHAPES = {
    "t64x3": (T64X3, 131, 301, 128),
    "t64x2": (T64X2, 1990, 1990, 128),
    "t128x2": (T128X2, 1990, 4099, 512),
    "8ph_row": (G8_ROW, 8348, 1700, 1024),
    "8ph_blk": (G8_BLK, 3841, 3850, 1024),
    "ws512_n128": (WS512, 16391, 128, 512),
    "ws512_n1024": (WS512, 16391, 1024, 512),
}
# bf16 outputs of >= 2^24 elements leave through non-temporal stores: id -> (kernel, M, N, K)
NT_SHAPES = {
    "nt_tile": (T64X2, 8192, 2048, 64),
    "nt_8ph": (G8_BLK, 8192, 2048, 1024),
    "nt_ws512": (WS512, 16391, 1024, 512),
}
TAP_SHAPES = [(200, C, taps, dil, N) for (taps, dil) in ((3, 1), (3, 2), (3, 4), (5, 1)) for C in (64, 128, 512) for N in (100, 512)]
TAP_BIG = (4100, 128, 5, 2, 2001)  # selects the 128 x 128 kernel (33 x 16 tiles, K = 640)
CONV2D_SHAPES = [(1, 3, 3, 64, 100), (2, 21, 9, 64, 128)]
SPLITK_M, SPLITK_NS = 131, (301, 256)
