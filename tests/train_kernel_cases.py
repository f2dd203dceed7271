"""Inputs, float64 references, comparators and planted defects of the element-wise tests of the training-step kernels
(mindaudio_amd/csrc/train_kernels.hip; test_train_kernel_cases_cpu.py, test_train_kernels_exact_gpu.py).  Nothing here needs a device.

THE DROPOUT MASK (train_common.h: drop_quad_hash, keep_elem, drop4, make_drop).  The keep decision of element `idx` of dropout site
`salt` at step seed `seed` is a pure function; every kernel of a site regenerates it.  keep_mask() restates it in uint32 / uint64 NumPy
arithmetic from the header's comment and code: ONE hash of two 32-bit words per element quad (idx >> 2), 16 bits per element (element
0 / 1 = low / high half of the first word, 2 / 3 = low / high half of the second), the element is kept when its 16 bits are
>= thresh >> 16, and the high word of the quad index (non-zero from 2^34 elements on) is folded into the first word without a multiply.
drop_params() restates make_drop: thresh = uint32(p * 2^32) (p as the float32 the launch receives, saturated at 2^32 - 1),
inv_keep = float32(1) / (float32(1) - float32(p)), p <= 0: no dropout.  Consequences:
  * only the upper 16 bits of thresh take part, so the REAL drop probability is floor(p * 2^16) / 2^16, not p;
  * for 0 < p < 2^-16 thresh is non-zero and thresh >> 16 is zero: nothing is ever dropped, yet every element is still scaled by
    inv_keep = 1 / (1 - p) (the kernels test `thresh`, not `thresh >> 16`, to decide whether dropout is on).
A site's kept value is its undropped float32 result times inv_keep (one float32 multiply), then the store's rounding; a dropped one is +0.

SITE INDICES (what each kernel documents, and what site_index() builds):
  act_dropout_fwd / _bwd (bf16 and _x32)   the flat element index
  dropout_add, dropout_bwd                 r * cols + c (NOT the row stride of any operand)
  layernorm_bwd_next's dy_next             row * 256 + column
  dense_act_drop / _bwd, ffn_train hidden  mc * N + n (N = the width of the output, not its row stride)
  dense_join, ffn_train join               mc * 256 + n
The GEMM sites run on small-integer operands (gemm_cases.int_matrix): the products are exact in any order of the sums.

BOUNDS.  u = 2^-24, a bf16 step is 2^-8 relative.  Exact sites (ReLU, dropout_add, dropout_bwd, dy_next, relu_bwd, im2col_t, col2im
on integers, the bf16 mirror, grad_overflow, refusals) are compared bit for bit.  The others:
  Swish sites: sigmoid_fast is v_rcp_f32(1 + v_exp_f32(-x log2 e)), the chain gemm_cases.act_bound was derived for:
      relative error of the sigmoid  rho(y) = u (2 (|y| + 1) (1 - sigmoid(y)) + 3)  <= 2^-21.6 for the inputs used here (|y| <= 12),
      far below the cap of 2^-12 a measured constant would be held to.  The float32 mode (1 / (1 + expf(-x)), expf within 2 ULP, the
      division within 2.5 ULP) is held to rho32 = u (4 (1 - sigmoid) + 6).  Backward: act' = s + y s (1 - s), d act' / d s = 1 + y (1 - 2 s),
      so |act' error| <= rho s |1 + y (1 - 2 s)| + 4 u (s + |y| s (1 - s)); times |dh|, one more rounding.
  LayerNorm backward (ln_bwd_bound): the derivation stands at the function.
  bn_finalize (bn_finalize_bound), Adam (adam_bound), the conv module's z and partial sums (conv_z_bound, conv_sums_bound): at the
  functions.  bn_finalize's variance is the ONE-PASS E[z^2] - mean^2, whose error grows like u n_eff (1 + mean^2 / sigma^2): with
  float32 chains (n_eff = 81) the derived bound of rstd at |mean| / sigma = 32 over 16 320 frames was 2^-7, above half a bf16 step
  (2^-9).  The forward kernel now adds with compensation and the finalize in double (n_eff = 3): 2^-12 (bn_onepass_case).

DEFECTS.  `defect=` on the references reproduces the mistakes these kernels could make; the CPU test shows that each fails the check_*
the GPU test uses, and that a float32 restatement of the correct operation passes it.
"""
import math

import numpy as np
import torch

import gemm_cases as G

U = G.U
ACT_SWISH, ACT_RELU = 1, 2
EPS_LN = 1e-5
LN_ROWS = (1, 3, 5, 4099)
LN_WIDTHS = (256, 512, 768, 1024)
LN_BLOCKS = 1024  # kLnBwdBlocks: workgroups (4 rows each per round) of a LayerNorm backward launch
DROP_PS = (0.1, 0.5)
P_TINY = 1e-5  # thresh != 0, thresh >> 16 == 0
SEED_SALTS = ((77, 5), (0x9E3779B9, 0xFFFFFFFF))
DEFECTS = ("mask_index_ld", "mask_pair_swapped", "row_scale_missing", "partials_last_group_dropped", "bn_unbiased_in_rstd",
           "relu_at_zero_passes", "col2im_even_edge", "adam_ignores_overflow", "mirror_truncates", "taps_flipped",
           "halo_crosses_utterance", "last_strip_dropped", "dsum_not_divided")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def f32(v):
    """The float32 value a launch receives for the Python float v, as a Python float."""
    return float(np.float32(v))


# ---- the mask ----------------------------------------------------------------------------------------------------------------------
def drop_params(p):
    """make_drop: (thresh, inv_keep) with thresh a Python int of 32 bits and inv_keep a numpy float32."""
    p32 = np.float32(p)
    if not p32 > 0:
        return 0, np.float32(1.0)
    th = float(p32) * 4294967296.0
    thresh = 0xFFFFFFFF if th >= 4294967295.0 else int(th)
    with np.errstate(divide="ignore"):
        return thresh, np.float32(1.0) / (np.float32(1.0) - p32)


def real_drop_probability(p):
    return (drop_params(p)[0] >> 16) / 65536.0


_M32 = np.uint64(0xFFFFFFFF)


def _mul32(x, k):
    return (x * np.uint64(k)) & _M32


def quad_hash(seed, salt, quad):
    """drop_quad_hash: quad (uint64 array) -> the two 32-bit words (uint64 arrays holding 32-bit values)."""
    quad = np.asarray(quad, dtype=np.uint64)
    hi = quad >> np.uint64(32)
    s = np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF) ^ np.uint64((int(salt) * 0x85EBCA6B) & 0xFFFFFFFF)
    x = (quad & _M32) ^ s ^ ((hi << np.uint64(16)) & _M32) ^ (hi >> np.uint64(16)) ^ hi
    x ^= x >> np.uint64(16)
    x = _mul32(x, 0x7FEB352D)
    x ^= x >> np.uint64(15)
    x = _mul32(x, 0x846CA68B)
    x ^= x >> np.uint64(16)
    y = x ^ np.uint64(0x9E3779B9)
    y = _mul32(y, 0xC2B2AE35)
    y ^= y >> np.uint64(15)
    return x, y


def keep_mask(seed, salt, idx, p, defect=None):
    """keep_elem for every element index of `idx` (any integer array / tensor; values up to 2^64 - 1) -> bool ndarray.
    p <= 0: everything is kept."""
    idx = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx).astype(np.uint64)
    thresh, _ = drop_params(p)
    if thresh == 0:
        return np.ones(idx.shape, dtype=bool)
    x, y = quad_hash(seed, salt, idx >> np.uint64(2))
    w = np.where((idx & np.uint64(2)) != 0, y, x)
    odd = (idx & np.uint64(1)) != 0
    if defect == "mask_pair_swapped":
        odd = ~odd
    bits = np.where(odd, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return bits >= np.uint64(thresh >> 16)


def site_index(rows, cols, ld=None, defect=None):
    """(rows, cols) int64 tensor of r * cols + c: the index of dropout_add / dropout_bwd / dy_next.  mask_index_ld: r * ld + c."""
    stride = ld if defect == "mask_index_ld" and ld is not None else cols
    return torch.arange(rows, dtype=torch.int64)[:, None] * stride + torch.arange(cols, dtype=torch.int64)[None, :]


# ---- number formats ----------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 tensor -> bf16, round to nearest even (the stores' conversion)."""
    return x.float().bfloat16()


def store_round(x, out_dtype, defect=None):
    if out_dtype == torch.bfloat16:
        return G.truncate_bf16(x) if defect == "mirror_truncates" else bf16_rne(x)
    return x.float()


def away_from_zero(shape, seed, lo=2.0 ** -3, hi=4.0, bf16=True, positive=False):
    """Random values with lo <= |v| <= hi (bf16-representable when bf16), either sign unless positive."""
    g = _gen(seed)
    v = lo + (hi - lo) * torch.rand(shape, generator=g)
    if not positive:
        v = v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    if bf16:
        v = v.bfloat16().float()
        v = torch.where(v.abs() < lo, torch.full_like(v, lo) * torch.sign(v), v)
    return v


# ---- comparators -------------------------------------------------------------------------------------------------------------------
def _positions(bad, limit=5):
    return [tuple(int(i) for i in p) for p in bad.nonzero()[:limit]]


def check_exact(got, case):
    """got must equal case["want"] bit for bit (same dtype) -> (0 or inf, positions)."""
    want = case["want"]
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = G._bits(got.contiguous().cpu()) != G._bits(want.contiguous())
    return (math.inf if bool(bad.any()) else 0.0), _positions(bad)


def check_bound(got, case):
    """|got - case["want"]| / case["bound"] per element (float64 want and bound; a bound of 0 demands equality) -> (worst, positions)."""
    want, bound = case["want"], case["bound"]
    err = (got.double().cpu() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    ratio = torch.where(torch.isfinite(got.double().cpu()), ratio, torch.full_like(ratio, math.inf))
    bad = ratio > 1
    return float(ratio.max()), _positions(bad)


def check_drop_site(got, case):
    """A dropout site's output: got == 0 (of either sign: 0 * -x is -0) where the restated mask drops or the undropped result is zero, and
    lo <= got <= hi (case["lo"], case["hi"] in the output's dtype; equal for an exact site) with got != 0 where it keeps.
    -> (worst |got - mid| / halfwidth over the kept elements with lo < hi, or inf on any violation, positions)."""
    got = got.cpu()
    lo, hi, nz = case["lo"], case["hi"], case["nonzero"]
    assert got.dtype == lo.dtype and got.shape == lo.shape, (got.dtype, lo.dtype, got.shape, lo.shape)
    gd, lod, hid = got.double(), lo.double(), hi.double()
    bad = torch.where(nz, ~((gd >= lod) & (gd <= hid)) | (gd == 0), gd != 0)
    if bool(bad.any()):
        return math.inf, _positions(bad)
    half = (hid - lod) / 2
    wide = nz & (half > 0)
    worst = float(((gd - (lod + hid) / 2).abs()[wide] / half[wide]).max()) if bool(wide.any()) else 0.0
    return worst, []


def _drop_window(ref, bound, keep, inv_keep, out_dtype, defect=None):
    """lo / hi / nonzero of a site whose undropped float32 result lies within ref +- bound (float64; bound None or 0: ref is the exact
    float32 value): the interval ends are scaled by inv_keep in float32 and rounded as the store does (both monotone)."""
    keep = torch.from_numpy(np.ascontiguousarray(keep)).view(ref.shape)
    ik = torch.tensor(float(inv_keep), dtype=torch.float32)
    if bound is None:
        assert bool((ref.float().double() == ref).all()), "an exact site's undropped result must be a float32 value"
        lo32 = hi32 = ref.float()
    else:
        b = bound + ref.abs() * 2.0 ** -23
        lo32, hi32 = (ref - b).float(), (ref + b).float()
    a, z = store_round(lo32 * ik, out_dtype, defect), store_round(hi32 * ik, out_dtype, defect)
    lo, hi = torch.minimum(a, z), torch.maximum(a, z)
    zero = torch.zeros_like(lo)
    nz = keep & (ref != 0)
    return {"lo": torch.where(nz, lo, zero), "hi": torch.where(nz, hi, zero), "nonzero": nz}


# ---- Swish / ReLU + dropout --------------------------------------------------------------------------------------------------------
def rho_fast(y):
    return G._rho(y)


def rho_f32(y):
    return U * (4.0 * (1.0 - torch.sigmoid(y)) + 6.0)


def act_fwd_ref(u, act, dt=torch.float64):
    u = u.to(dt)
    return u.clamp(min=0) if act == ACT_RELU else u * torch.sigmoid(u)


def act_grad_ref(u, act, dt=torch.float64, defect=None):
    """act'(u): ReLU: 1 for u > 0 (0 at +-0); relu_at_zero_passes: 1 for u >= 0."""
    u = u.to(dt)
    if act == ACT_RELU:
        return ((u >= 0) if defect == "relu_at_zero_passes" else (u > 0)).to(dt)
    s = torch.sigmoid(u)
    return s + u * s * (1 - s)


def act_fwd_bound(u, act, x32):
    if act == ACT_RELU:
        return None
    u = u.double()
    rho = rho_f32(u) if x32 else rho_fast(u)
    return 1.001 * (u * torch.sigmoid(u)).abs() * (rho + U) + 2.0 ** -126


def act_bwd_bound(u, dh, act, x32):
    if act == ACT_RELU:
        return None
    u, dh = u.double(), dh.double()
    s = torch.sigmoid(u)
    rho = rho_f32(u) if x32 else rho_fast(u)
    dact = rho * s * (1 + u * (1 - 2 * s)).abs() + 4 * U * (s + u.abs() * s * (1 - s))
    return 1.001 * (dh.abs() * dact + U * (dh * (s + u * s * (1 - s))).abs()) + 2.0 ** -126


def act_dropout_case(n, act, p, seed, salt, x32, backward, data_seed=11, defect=None):
    """u (n,) with |u| >= 2^-3 (Swish: u >= 1, so that out != 0 reads the mask), dh likewise; bf16 values unless x32."""
    u = away_from_zero((n,), data_seed, lo=1.0 if act == ACT_SWISH else 2.0 ** -3, hi=8.0, bf16=not x32, positive=act == ACT_SWISH)
    dh = away_from_zero((n,), data_seed + 1, bf16=not x32)
    thresh, inv_keep = drop_params(p)
    keep = keep_mask(seed, salt, np.arange(n, dtype=np.uint64), p, defect)
    if backward:
        ref = dh.double() * act_grad_ref(u, act, defect=defect)
        bound = act_bwd_bound(u, dh, act, x32)
    else:
        ref, bound = act_fwd_ref(u, act), act_fwd_bound(u, act, x32)
    case = {"u": u, "dh": dh, "n": n, "act": act, "p": p, "seed": seed, "salt": salt, "x32": x32, "backward": backward,
            "undropped": ref}
    case.update(_drop_window(ref, bound, keep, inv_keep, torch.float32 if x32 else torch.bfloat16))
    return case


def act_dropout_f32(case, keep=None):
    """float32 restatement (precise sigmoid) -> the output in the case's dtype."""
    u, dh = case["u"].float(), case["dh"].float()
    if case["backward"]:
        v = dh * act_grad_ref(u, case["act"], dt=torch.float32)
    else:
        v = act_fwd_ref(u, case["act"], dt=torch.float32)
    thresh, inv_keep = drop_params(case["p"])
    if keep is None:
        keep = keep_mask(case["seed"], case["salt"], np.arange(case["n"], dtype=np.uint64), case["p"])
    if thresh:
        v = torch.where(torch.from_numpy(keep), v * torch.tensor(float(inv_keep)), torch.zeros_like(v))
    return store_round(v, torch.float32 if case["x32"] else torch.bfloat16)


# ---- dropout_add / dropout_bwd -----------------------------------------------------------------------------------------------------
def dropout_add_case(rows, cols, y_bf16, with_x, p, seed, salt, alpha=0.5, ld=None, data_seed=21, defect=None):
    """out = x + alpha * dropout(y), row strides left to the caller.  alpha is a power of two, so alpha * v is exact and
    fl(x + fl(alpha v)) is the one value a compiler can produce, with or without a fused multiply-add: `want` holds it bit for bit
    (v = fl(y * inv_keep) where the restated mask keeps, 0 where it drops)."""
    y = away_from_zero((rows, cols), data_seed, bf16=y_bf16)
    x = (torch.randint(-512, 512, (rows, cols), generator=_gen(data_seed + 1)).float() / 64.0) if with_x else None
    thresh, inv_keep = drop_params(p)
    keep = torch.from_numpy(keep_mask(seed, salt, site_index(rows, cols, ld, defect), p, defect if defect != "mask_index_ld" else None))
    v = y.float() * torch.tensor(float(inv_keep)) if thresh else y.float()
    v = torch.where(keep, v, torch.zeros_like(v))
    want = (x if with_x else torch.zeros_like(v)) + torch.tensor(alpha, dtype=torch.float32) * v  # alpha * v exact: one rounding
    return {"x": x, "y": bf16_rne(y) if y_bf16 else y, "rows": rows, "cols": cols, "alpha": alpha, "p": p, "seed": seed, "salt": salt,
            "want": want, "keep": keep}


def dropout_bwd_case(rows, cols, x32, p, seed, salt, alpha=0.5, ld=None, data_seed=31, defect=None):
    """dy = alpha * keep / (1 - p) * g * row_scale; row_scale in {0, 0.5, 1} with zero rows, alpha a power of two: the undropped value
    is an exact float32 number."""
    g = away_from_zero((rows, cols), data_seed, bf16=False)
    rs = torch.tensor([0.0, 1.0, 0.5])[torch.randint(0, 3, (rows,), generator=_gen(data_seed + 1))]
    rs[0] = 0.0
    ref = g.double() * alpha * (1.0 if defect == "row_scale_missing" else rs.double()[:, None])
    thresh, inv_keep = drop_params(p)
    keep = keep_mask(seed, salt, site_index(rows, cols, ld, defect), p, defect if defect != "mask_index_ld" else None)
    case = {"g": g, "row_scale": rs, "rows": rows, "cols": cols, "alpha": alpha, "p": p, "seed": seed, "salt": salt, "x32": x32}
    case.update(_drop_window(ref, None, keep, inv_keep, torch.float32 if x32 else torch.bfloat16))
    return case


def dy_next_case(g_out, alpha, rs_next, p, seed, salt, ld=None, defect=None):
    """layernorm_bwd_next's second output from the float32 rows g_out the SAME launch stored: bf16(dropout(g * alpha * rs_next))."""
    rows, cols = g_out.shape
    v = g_out.float() * torch.tensor(alpha, dtype=torch.float32)
    if rs_next is not None and defect != "row_scale_missing":
        v = v * rs_next.float()[:, None]
    thresh, inv_keep = drop_params(p)
    keep = keep_mask(seed, salt, site_index(rows, cols, ld, defect), p, defect if defect != "mask_index_ld" else None)
    return _drop_window(v.double(), None, keep, inv_keep, torch.bfloat16)


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------
def ln_last_round_rows(rows):
    """Rows of the last persistent round of layernorm_bwd_kernel: grid = min(ceil(rows / 4), 1024) workgroups of 4 waves."""
    per_round = min((rows + 3) // 4, LN_BLOCKS) * 4
    return (rows - 1) // per_round * per_round


def ln_bwd_ref(x, gamma, dy, g0, row_scale=None, accumulate=True, eps=EPS_LN, dt=torch.float64, defect=None):
    """-> (g, dgamma, dbeta, parts) of y = ((x - mu) rstd gamma + beta) row_scale; parts = what the bounds need (float64 only)."""
    x, gamma, dy = x.to(dt), gamma.to(dt), dy.to(dt)
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xh = xc * rstd
    if row_scale is not None and defect != "row_scale_missing":
        dy = dy * row_scale.to(dt)[:, None]
    w = dy * gamma
    a = w.mean(-1, keepdim=True)
    b = (w * xh).mean(-1, keepdim=True)
    e = w - a - xh * b
    dx = rstd * e
    g = g0.to(dt) + dx if accumulate else dx
    tg, tb = dy * xh, dy
    if defect == "partials_last_group_dropped":
        first = ln_last_round_rows(x.shape[0])
        tg, tb = tg[:first], tb[:first]
    return g, tg.sum(0), tb.sum(0), {"mu": mu, "xc": xc, "var": var, "rstd": rstd, "xh": xh, "dy": dy, "w": w, "a": a, "b": b, "e": e}


def ln_bwd_bound(x, gamma, dy, g0, row_scale, accumulate, dg0, db0, eps=EPS_LN, depth=None):
    """Per-element bound of g and per-column bounds of dgamma / dbeta for the kernels' float32 arithmetic (both the 256-wide and the
    wide kernel; D the width, d = D / 64 + 7 the depth of a row sum: D / 64 in-lane additions, six shuffles, the scaling by the
    rounded 1 / D).  With gam(k) = k u / (1 - k u), all right-hand sides exact (float64) quantities:
        mean:   dm = gam(d) mean|x|
        x - mu: dd_i = dm + u (|x_i - mu| + dm)
        var:    dV = gam(d + 2) mean((|x_i - mu| + dd_i)^2) + mean(2 |x_i - mu| dd_i + dd_i^2);  T = var + eps, dT = dV + u (T + dV)
        rstd:   rho = (1 - dT / T)^-1/2 - 1 + 9 u      (sqrtf and the division, as packed_cases.ln_bound)
        xhat:   dx_i = rstd dd_i (1 + rho) + |xhat_i| (rho + u)
        w = dy gamma: u |w_i|;  a: da = (gam(d) + u) mean|w|;  b: db = gam(d + 2) mean|w xhat| + mean(|w_i| dx_i) (1 + 2 u)
        e_i = w_i - a - xhat_i b:  de_i = u |w_i| + da + |xhat_i| db + |b| dx_i + dx_i db + 3 u (|w_i| + |a| + |xhat_i b|)
        g_i = g0_i + rstd e_i:     rstd de_i (1 + rho) + |rstd e_i| (rho + 2 u) + u |g_i|
    dgamma_c = dgamma0_c + sum_rows dy xhat: every term carries |dy| dx_i + u |dy xhat|; the sum runs through at most S = 48 additions
    (rows of a wave in sequence, 4 waves, then partial_reduce_kernel's 4 interleaved chains of <= 16 and its 16 row groups):
        gam(S) sum|dy xhat| + sum(|dy| dx_i) + u |dgamma_c|;   dbeta likewise without the xhat terms.
    All times 1.001 for the second-order terms, plus 2^-126."""
    D = x.shape[1]
    d = depth if depth is not None else D // 64 + 7  # (the GEMM epilogues add a row in another order: EPI_LN_DEPTH)

    def gam(k):
        return k * U / (1 - k * U)

    _, dgr, dbr, q = ln_bwd_ref(x, gamma, dy, g0, row_scale, accumulate, eps)
    xd = x.double()
    dm = gam(d) * xd.abs().mean(-1, keepdim=True)
    axc = q["xc"].abs()
    dd = dm + U * (axc + dm)
    dV = gam(d + 2) * ((axc + dd) ** 2).mean(-1, keepdim=True) + (2 * axc * dd + dd * dd).mean(-1, keepdim=True)
    T = q["var"] + f32(eps)
    dT = dV + U * (T + dV)
    assert bool((dT < 0.5 * T).all()), "the variance is lost in its own rounding: choose other rows"
    rho = (1 - dT / T) ** -0.5 - 1 + 9 * U
    rstd, xh, w, a, b, e = q["rstd"], q["xh"], q["w"], q["a"], q["b"], q["e"]
    dx = rstd * dd * (1 + rho) + xh.abs() * (rho + U)
    da = (gam(d) + U) * w.abs().mean(-1, keepdim=True)
    db = gam(d + 2) * (w * xh).abs().mean(-1, keepdim=True) + (w.abs() * dx).mean(-1, keepdim=True) * (1 + 2 * U)
    de = U * w.abs() + da + xh.abs() * db + b.abs() * dx + dx * db + 3 * U * (w.abs() + a.abs() + (xh * b).abs())
    gref = (g0.double() if accumulate else 0) + rstd * e
    bg = 1.001 * (rstd * de * (1 + rho) + (rstd * e).abs() * (rho + 2 * U) + U * gref.abs()) + 2.0 ** -126
    S = 48
    dyv = q["dy"]
    bdg = 1.001 * (gam(S) * (dyv * xh).abs().sum(0) + (dyv.abs() * dx).sum(0) + U * (dg0.double() + dgr).abs()) + 2.0 ** -126
    bdb = 1.001 * (gam(S) * dyv.abs().sum(0) + U * (db0.double() + dbr).abs()) + 2.0 ** -126
    return bg, bdg, bdb


def ln_bwd_case(rows, D, dy_bf16, accumulate, inplace=False, onehot=None, seed=41, defect=None):
    """x rows with a constant row, a row at 100 + N(0, 1) and a row of 1e-3 N(0, 1) among N(0.3, 2) rows; row_scale in {0, 0.5, 1}
    with zero rows; g0, dgamma0, dbeta0 non-zero.  inplace: dy is g itself (float32, accumulate off).  onehot: dy is non-zero in that
    row only and dgamma0 = dbeta0 = 0: dbeta must be the row exactly."""
    g = _gen(seed + 7 * rows + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.3
    if rows >= 3:
        x[0] = 0.7
        x[1] = 100.0 + torch.randn(D, generator=g)
        x[rows - 1] = 1e-3 * torch.randn(D, generator=g)
    elif rows == 1:
        x[0] = 100.0 + torch.randn(D, generator=g)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    if dy_bf16:
        dy = dy.bfloat16().float()
    rs = torch.tensor([0.0, 1.0, 0.5, 1.0])[torch.randint(0, 4, (rows,), generator=g)]
    if rows >= 3:
        rs[0], rs[1], rs[rows - 1] = 1.0, 1.0, 1.0  # the special rows take part
        if rows > 3:
            rs[2] = 0.0
    else:
        rs[0] = 1.0
    g0 = torch.randn(rows, D, generator=g)
    dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    if onehot is not None:
        dy = torch.where(torch.arange(rows)[:, None] == onehot, dy, torch.zeros_like(dy))
        rs[onehot] = 1.0
        dg0, db0 = torch.zeros(D), torch.zeros(D)
    if inplace:
        accumulate, g0 = False, dy.clone()
    gref, dgr, dbr, _ = ln_bwd_ref(x, gamma, dy, g0, rs, accumulate, defect=defect)
    bg, bdg, bdb = ln_bwd_bound(x, gamma, dy, g0, rs, accumulate, dg0, db0)
    return {"x": x, "gamma": gamma, "dy": dy, "dy_bf16": dy_bf16, "row_scale": rs, "g0": g0, "dg0": dg0, "db0": db0, "rows": rows,
            "D": D, "accumulate": accumulate, "inplace": inplace, "onehot": onehot,
            "g": {"want": gref, "bound": bg},
            "dgamma": {"want": dg0.double() + dgr, "bound": bdg}, "dbeta": {"want": db0.double() + dbr, "bound": bdb},
            "dgamma_sum": {"want": dgr, "bound": bdg}, "dbeta_sum": {"want": dbr, "bound": bdb}}


def check_ln_bwd(got, case):
    """got = (g, dgamma, dbeta) as the launch left them (dgamma / dbeta: the accumulated buffers, or with case["partials"] the float64
    sums of the partial vectors) -> (worst error / bound, positions as (name, index...))."""
    g, dg, db = got
    worst, pos = 0.0, []
    names = ("g", "dgamma_sum" if case.get("partials") else "dgamma", "dbeta_sum" if case.get("partials") else "dbeta")
    for name, t in zip(names, (g, dg, db)):
        w, p = check_bound(t, case[name])
        worst = max(worst, w)
        pos += [(name,) + q for q in p]
    if case["onehot"] is not None:
        r = case["onehot"]
        # dbeta is the row itself; every other row of g is untouched (accumulate) or exactly zero
        w, p = check_exact(db.float().cpu(), {"want": (case["dy"][r] * case["row_scale"][r]).float()})
        worst = max(worst, w)
        pos += [("dbeta_onehot",) + q for q in p]
        others = torch.arange(case["rows"]) != r
        rest = case["g0"][others] if case["accumulate"] else torch.zeros_like(case["g0"][others])
        w, p = check_exact(g.float().cpu()[others], {"want": rest.float()})
        worst = max(worst, w)
        pos += [("g_other_rows",) + q for q in p]
    return worst, pos


def ln_bwd_f32(case):
    """float32 restatement of the kernel's formulas (two-pass statistics) -> (g, dgamma, dbeta)."""
    g, dg, db, _ = ln_bwd_ref(case["x"], case["gamma"], case["dy"], case["g0"], case["row_scale"], case["accumulate"], dt=torch.float32)
    if case.get("partials"):
        return g, dg.double(), db.double()
    return g, case["dg0"] + dg, case["db0"] + db


# ---- BatchNorm finalize ------------------------------------------------------------------------------------------------------------
BN_NPARTS = (1, 15, 16, 17, 112, 113, 128, 129, 300)
BN_CS = (16, 24, 256)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_finalize_ref(sums, count, C, run_mean, run_var, eps=BN_EPS, momentum=BN_MOMENTUM, dt=torch.float64, defect=None):
    """sums (nparts, 2 C): (sum | sum of squares) partial vectors -> (stats (2 C): mean | rstd, running mean, running variance):
    biased variance in rstd, running_var with the kernel's documented count / max(count - 1, 1)."""
    tot = sums.to(dt).sum(0)
    mean = tot[:C] / count
    var = (tot[C:] / count - mean * mean).clamp(min=0)
    unb = var * (count / max(count - 1.0, 1.0))
    mom = torch.tensor(f32(momentum), dtype=dt)
    rstd = 1.0 / torch.sqrt((unb if defect == "bn_unbiased_in_rstd" else var) + f32(eps))
    return torch.cat([mean, rstd]), (1 - mom) * run_mean.to(dt) + mom * mean, (1 - mom) * run_var.to(dt) + mom * unb


def _rnd(v, k=1.0):
    """k u |v| where v (float64) is not a float32 value, else 0: a correctly rounded operation whose exact result is representable
    returns it."""
    return torch.where(v.float().double() == v, torch.zeros_like(v), k * U * v.abs())


def bn_finalize_bound(sums, count, C, run_mean, run_var, eps=BN_EPS, momentum=BN_MOMENTUM, sum_rel=None, sum_abs=None):
    """The kernel adds the float32 partials and forms mean = a / count and var = max(q / count - mean^2, 0) in DOUBLE (its own
    rounding, 2^-53 per operation, is far below everything here), then rounds mean and var to float32 and takes
    rstd = 1 / sqrtf(var + eps).  What is left is the error the partials arrive with: none for the small integers of
    bn_finalize_case, sum_rel = (r1, r2) times u times sum_abs = (sum |z|, sum z^2) for a forward launch's compensated sums:
        dmean = r1 u sum|z| / count;  dE2 = r2 u sum z^2 / count;  dV = dE2 + 2 |mean| dmean + dmean^2 + u var   (the cast)
        mean: dmean + u |mean| (the cast);  rstd: T = var + eps, dT = dV + u T, rho = (1 - dT / T)^-1/2 - 1 + 9 u
        running mean: 4 u (|(1 - m) rm| + |m mean|) + m dmean';  running var: 6 u (|(1 - m) rv| + |m unb|) + m k dV, k = count / max(count - 1, 1)
    -> (bound of stats (2 C), bound of running mean, bound of running variance)."""
    tot = sums.double().sum(0)
    ds = torch.zeros(2 * C, dtype=torch.float64)
    if sum_rel is not None:
        ds = torch.cat([sum_rel[0] * U * sum_abs[:C], sum_rel[1] * U * sum_abs[C:]])
    mean, E2 = tot[:C] / count, tot[C:] / count
    dmean, dE2 = ds[:C] / count, ds[C:] / count
    var = (E2 - mean * mean).clamp(min=0)
    dV = dE2 + 2 * mean.abs() * dmean + dmean * dmean + U * var
    dmean = dmean + _rnd(mean)
    T = var + f32(eps)
    dT = dV + U * T
    rho = torch.where(dT < 0.75 * T, (1 - (dT / T).clamp(max=0.75)) ** -0.5 - 1, torch.full_like(T, math.inf)) + 9 * U
    rstd = 1.0 / torch.sqrt(T)
    k = count / max(count - 1.0, 1.0)
    mom = f32(momentum)
    brm = 4 * U * (((1 - mom) * run_mean.double()).abs() + (mom * mean).abs()) + mom * dmean
    brv = 6 * U * (((1 - mom) * run_var.double()).abs() + (mom * k * var).abs()) + mom * k * dV
    return 1.001 * torch.cat([dmean, rstd * rho]) + 2.0 ** -126, 1.001 * brm + 2.0 ** -126, 1.001 * brv + 2.0 ** -126


def bn_finalize_case(nparts, C, count=None, seed=51, defect=None):
    """Partial vectors of small integers (exactly summable in any order): channel c holds values v in {-3 .. 3} + a per-channel
    offset in {0, 1, 2}, one value per frame, `per` frames per partial; channel 1 is constant (its variance clamps at 0).
    count = 1: one partial, one frame."""
    g = _gen(seed + 1000 * nparts + C)
    per = 1 if count == 1 else 3
    if count is None:
        count = nparts * per
    assert count == nparts * per
    v = torch.randint(-3, 4, (nparts, per, C), generator=g).float() + torch.randint(0, 3, (C,), generator=g).float()
    v[:, :, 1] = 2.0
    sums = torch.cat([v.sum(1), (v * v).sum(1)], dim=1)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    stats, nrm, nrv = bn_finalize_ref(sums, count, C, rm, rv, defect=defect)
    bs, brm, brv = bn_finalize_bound(sums, count, C, rm, rv)
    return {"sums": sums, "nparts": nparts, "C": C, "count": count, "run_mean": rm, "run_var": rv,
            "stats": {"want": stats, "bound": bs}, "rm": {"want": nrm, "bound": brm}, "rv": {"want": nrv, "bound": brv}}


def check_bn_finalize(got, case):
    worst, pos = 0.0, []
    for name, t in zip(("stats", "rm", "rv"), got):
        w, p = check_bound(t, case[name])
        worst = max(worst, w)
        pos += [(name,) + q for q in p]
    return worst, pos


def bn_finalize_f32(case):
    """The kernel's arithmetic restated: sums, mean and E[z^2] - mean^2 in double, then float32."""
    C, count = case["C"], case["count"]
    tot = case["sums"].double().sum(0)
    mean = (tot[:C] / count)
    var = (tot[C:] / count - mean * mean).clamp(min=0).float()
    mean = mean.float()
    eps, mom = torch.tensor(BN_EPS, dtype=torch.float32), torch.tensor(BN_MOMENTUM, dtype=torch.float32)
    k = torch.tensor(count / max(count - 1.0, 1.0), dtype=torch.float32)
    return (torch.cat([mean, 1.0 / torch.sqrt(var + eps)]), (1 - mom) * case["run_mean"] + mom * mean,
            (1 - mom) * case["run_var"] + mom * var * k)


# ---- subsampling backward ----------------------------------------------------------------------------------------------------------
SUB_SHAPES = ((1, 3, 3, 8), (2, 4, 6, 72), (2, 21, 19, 64))  # (B, H, W, C): M % 64 != 0, C % 64 != 0, even H / W


def out_hw(h, w):
    return (h - 3) // 2 + 1, (w - 3) // 2 + 1


def relu_bwd_case(n=1003, x32=False, seed=61, defect=None):
    """dy *= (y > 0): y holds +0, -0, the smallest positive (subnormal) value of the format, the smallest normal one, their negatives."""
    g = _gen(seed)
    dy = away_from_zero((n,), seed, bf16=not x32)
    y = torch.randn(n, generator=g)
    if not x32:
        y = y.bfloat16().float()
    tiny = 2.0 ** -149 if x32 else 2.0 ** -133
    y[:8] = torch.tensor([0.0, -0.0, tiny, -tiny, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0])
    dt = torch.float32 if x32 else torch.bfloat16
    keep = (y >= 0) if defect == "relu_at_zero_passes" else (y > 0)
    return {"dy": dy.to(dt), "y": y.to(dt), "n": n, "want": torch.where(keep, dy, torch.zeros_like(dy)).to(dt)}


def im2col_t_ref(act):
    """act (B, H, W, C) -> (9 C, B Ho Wo): row (kh, kw, c), column (b, ho, wo)."""
    b, h, w, c = act.shape
    ho, wo = out_hw(h, w)
    rows = [act[:, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2, :].reshape(b * ho * wo, c).t() for kh in range(3) for kw in range(3)]
    return torch.cat(rows, 0)


def col2im_relu_ref(dcol, act, dt=torch.float64, defect=None):
    """dcol (B Ho Wo, 9 C), act (B, H, W, C) -> dact = (act > 0) * the sum of the <= 4 windows that contain the position."""
    b, h, w, c = act.shape
    ho, wo = out_hw(h, w)
    d = dcol.to(dt).view(b, ho, wo, 9, c)
    out = torch.zeros(b, h, w, c, dtype=dt)
    for kh in range(3):
        for kw in range(3):
            out[:, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2, :] += d[:, :, :, kh * 3 + kw, :]
    if defect == "col2im_even_edge":  # the bound ho < Ho forgotten: the last row / column of an even extent reads a window of padding
        if h % 2 == 0:
            out[:, h - 1, 0:2 * wo - 1:2, :] += d[:, ho - 1, :, 0, :]
        if w % 2 == 0:
            out[:, 0:2 * ho - 1:2, w - 1, :] += d[:, :, wo - 1, 0, :]
    gate = (act >= 0) if defect == "relu_at_zero_passes" else (act > 0)
    return out * gate.to(dt)


def subsample_case(shape, x32=False, seed=71, defect=None):
    """act: small integers with zeros of both signs; dcol: integers in {-8 .. 8} (sums of <= 4 are exact in bf16)."""
    b, h, w, c = shape
    g = _gen(seed + h * w + c)
    ho, wo = out_hw(h, w)
    act = torch.randint(-3, 4, shape, generator=g).float()
    act = torch.where((act == 0) & (torch.rand(shape, generator=g) < 0.5), torch.full_like(act, -0.0), act)
    dcol = torch.randint(-8, 9, (b * ho * wo, 9 * c), generator=g).float()
    dcol = torch.where(dcol == 0, torch.ones_like(dcol), dcol)  # no zeros: a window that must not arrive always shows
    dt = torch.float32 if x32 else torch.bfloat16
    want = col2im_relu_ref(dcol, act, defect=defect)
    return {"shape": shape, "act": act.to(dt), "dcol": dcol.to(dt), "m": b * ho * wo,
            "im2col": {"want": im2col_t_ref(act).to(dt)}, "col2im": {"want": (want + 0.0).to(dt)}}


# ---- optimizer ---------------------------------------------------------------------------------------------------------------------
OVERFLOW_N = 2048 * 256 + 3
ADAM_HP = dict(lr_t=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, inv_scale=1.0 / 1024)


def overflow_ref(g):
    return int(bool((~torch.isfinite(g)).any()))


def adam_ref(p, g, m, v, lr_t, beta1, beta2, eps, inv_scale, overflow=0, dt=torch.float64, defect=None):
    """nn.Adam with the float32 hyper-parameters the launch receives; (1 - beta) is exact in float32 (Sterbenz)."""
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    if overflow and defect != "adam_ignores_overflow":
        return p, m, v
    b1, b2 = f32(beta1), f32(beta2)
    gi = g * f32(inv_scale)
    mi = b1 * m + (1.0 - b1) * gi
    vi = b2 * v + (1.0 - b2) * gi * gi
    return p - f32(lr_t) * mi / (torch.sqrt(vi) + f32(eps)), mi, vi


def adam_bound(p, g, m, v, lr_t, beta1, beta2, eps, inv_scale):
    """inv_scale is a power of two (gi exact).  m' = b1 m + c1 gi: two products and a sum: 2 u (|b1 m| + |c1 gi|).
    v' = b2 v + c2 gi gi: 4 u (|b2 v| + c2 gi^2).  s = sqrtf(v') within 2 u relative: ds = s (dv' / (2 v') + 2 u) (0 at v' = 0);
    d = s + eps: dd = ds + u d;  num = lr_t m': dnum = lr_t dm' + u |num|;  step = num / d (3 u):
    dstep = |step| (dd / d + 3 u) + dnum / d;  p' = p - step: dstep + u |p'|.  Times 1.001, plus 2^-126 (2^-149 for v': gi^2 may be
    subnormal)."""
    pn, mi, vi = adam_ref(p, g, m, v, lr_t, beta1, beta2, eps, inv_scale)
    b1, b2 = f32(beta1), f32(beta2)
    gi = g.double() * f32(inv_scale)
    bm = 2 * U * ((b1 * m.double()).abs() + ((1 - b1) * gi).abs())
    bv = 4 * U * ((b2 * v.double()).abs() + (1 - b2) * gi * gi) + 2.0 ** -149
    s = torch.sqrt(vi)
    ds = torch.where(vi > 0, s * (bv / (2 * vi.clamp(min=1e-300)) + 2 * U), torch.sqrt(bv))
    d = s + f32(eps)
    dd = ds + U * d
    num = f32(lr_t) * mi
    dnum = f32(lr_t) * bm + U * num.abs()
    step = num / d
    bstep = step.abs() * (dd / d + 3 * U) + dnum / d
    bp = bstep + U * pn.abs()
    return 1.001 * bp + 2.0 ** -126, 1.001 * bm + 2.0 ** -126, 1.001 * bv + 2.0 ** -126


def adam_case(n, seed=81, lr_t=None, overflow=0, defect=None):
    """Random p, g (scaled by 1024), m, v >= 0; element 0 has v = g = m = 0 (a step of exactly 0, not NaN); with lr_t = 0 the new
    p is p itself and p holds bf16 ties of both parities (low half 0x8000) for the mirror."""
    g_ = _gen(seed + n)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_) * 1024
    m, v = 0.1 * torch.randn(n, generator=g_), 0.01 * torch.rand(n, generator=g_)
    g[0], m[0], v[0] = 0.0, 0.0, 0.0
    hp = dict(ADAM_HP)
    if lr_t is not None:
        hp["lr_t"] = lr_t
    if hp["lr_t"] == 0.0:
        bits = p.view(torch.int32)
        k = min(n, 64)
        bits[:k] = (bits[:k] & -65536) | 0x8000  # exactly halfway; the kept upper halves are odd and even
        p = bits.view(torch.float32)
    pn, mn, vn = adam_ref(p, g, m, v, overflow=overflow, defect=defect, **hp)
    bp, bm, bv = adam_bound(p, g, m, v, **hp)
    if overflow:
        bp, bm, bv = torch.zeros_like(bp), torch.zeros_like(bm), torch.zeros_like(bv)
    return {"p": p, "g": g, "m": m, "v": v, "n": n, "hp": hp, "overflow": overflow,
            "pn": {"want": pn, "bound": bp}, "mn": {"want": mn, "bound": bm}, "vn": {"want": vn, "bound": bv}}


def check_adam(got, case):
    """got = (p, m, v[, mirror]) after the launch: p, m, v within the bounds (bit-unchanged on overflow: bounds of 0); the mirror is the
    round-to-nearest-even bf16 of the p the launch stored (or, on overflow, what it held before: case["mirror0"])."""
    worst, pos = 0.0, []
    for name, t in zip(("pn", "mn", "vn"), got[:3]):
        w, q = check_bound(t, case[name])
        worst = max(worst, w)
        pos += [(name,) + x for x in q]
    if len(got) > 3:
        want = case["mirror0"] if case["overflow"] else bf16_rne(got[0].cpu())
        w, q = check_exact(got[3].cpu(), {"want": want})
        worst = max(worst, w)
        pos += [("mirror",) + x for x in q]
    return worst, pos


def adam_f32(case, mirror=False, defect=None):
    hp = case["hp"]
    p, m, v = adam_ref(case["p"], case["g"], case["m"], case["v"], overflow=case["overflow"], dt=torch.float32, defect=defect, **hp)
    out = (p, m, v)
    if mirror:
        unchanged = case["overflow"] and defect != "adam_ignores_overflow"
        out += (case["mirror0"] if unchanged else store_round(p, torch.bfloat16, defect),)
    return out


# ---- training conv module, forward -------------------------------------------------------------------------------------------------
CONV_KS = (3, 7, 15, 31)
CONV_TS = (1, 5, 16, 17, 33, 47)  # T < pad (every halo load is clamped), one strip, a strip + 1, two strips + 1, a ragged third
CONV_CS = (256, 512)
CONV_FRAMES_PER_PART = 32  # kCfStrip * kCfPerBlock: frames a forward workgroup adds into its partial (sum | sum of squares) vector


def convmid_fwd_ref(y, B, T, C, w, bias, dt=torch.float64, defect=None):
    """y (B T, 2 C) = (a | gate) -> z (B T, C) = bias + sum_j w[c][j] glu(y)[b, t + j - pad, c] (zero outside the utterance), and glu(y)."""
    y = y.to(dt).view(B, T, 2 * C)
    s = y[..., :C] * torch.sigmoid(y[..., C:])
    ks = w.shape[1]
    pad = (ks - 1) // 2
    wv = w.to(dt).flip(1) if defect == "taps_flipped" else w.to(dt)
    rows = s.reshape(1, B * T, C) if defect == "halo_crosses_utterance" else s
    n = rows.shape[1]
    sp = torch.nn.functional.pad(rows, (0, 0, pad, pad))
    z = bias.to(dt) + sum(wv[:, j] * sp[:, j:j + n] for j in range(ks))
    z = z.reshape(B, T, C).clone()
    if defect == "last_strip_dropped" and T % 16:
        z[:, T // 16 * 16:] = 0
    return z.reshape(B * T, C), s.reshape(B * T, C)


def conv_route_case(ks, T, C, x32, defect=None):
    """Routing, exact: gate = +40 everywhere (sigmoid = 1), `a` zero except ONE power-of-two impulse per channel, at (utterance, frame)
    = ROUTE[c % 6] of B = 3 utterances (the middle one all zero, between an impulse in the last frame of utterance 0 and one in the first
    frame of utterance 2); w[c][j] = 2^-(j + c mod 5), bias[c] = 2^(c mod 3).  Every tap but one multiplies a zero, so
    z[b, t, c] = fl32(bias + w[c][t0 - t + pad] a) inside the footprint (one rounding: the fused multiply-add) and the bias outside it."""
    B = 3
    route = ((0, T - 1), (2, 0), (0, min(15, T - 1)), (2, min(16, T - 1)), (0, 0), (2, T - 1))
    y = torch.zeros(B, T, 2 * C)
    y[..., C:] = 40.0
    for c in range(C):
        b, t = route[c % 6]
        y[b, t, c] = 2.0 ** (1 + c % 2)
    j = torch.arange(ks, dtype=torch.float64)
    w = torch.exp2(-(j[None, :] + (torch.arange(C) % 5)[:, None].double())).float()
    bias = torch.exp2((torch.arange(C) % 3).double()).float()
    z, _ = convmid_fwd_ref(y.view(B * T, 2 * C), B, T, C, w, bias, defect=defect)
    assert defect is not None or float(z.view(B, T, C)[1].sub(bias.double()).abs().max()) == 0.0  # the middle utterance: the bias
    return {"y": y.view(B * T, 2 * C).to(torch.float32 if x32 else torch.bfloat16), "B": B, "T": T, "C": C, "ks": ks, "w": w,
            "bias": bias, "want": z.float()}


def conv_random_case(ks, T, C, x32, B=3, seed=91, bias_ratio=None):
    """Random (a | gate), w ~ 0.3 N(0, 1), bias ~ 0.1 N(0, 1) - or, with bias_ratio (C,), bias = ratio * the channel's float64 standard
    deviation of z, so that |mean| / sigma of the BatchNorm input is about the ratio (the one-pass variance case)."""
    g = _gen(seed + ks + 100 * T + C)
    y = torch.randn(B * T, 2 * C, generator=g)
    if not x32:
        y = y.bfloat16().float()
    w, bias = 0.3 * torch.randn(C, ks, generator=g), 0.1 * torch.randn(C, generator=g)
    if bias_ratio is not None:
        z0, _ = convmid_fwd_ref(y, B, T, C, w, torch.zeros(C))
        bias = (bias_ratio.double() * z0.std(0, unbiased=False) - z0.mean(0)).float()
    return {"y": y.to(torch.float32 if x32 else torch.bfloat16), "B": B, "T": T, "C": C, "ks": ks, "w": w, "bias": bias, "x32": x32}


def conv_z_bound(case):
    """(z64, bound): the kernel forms s = a * sigmoid(gate) in float32 (relative error rho + u, rho of the mode's sigmoid) and
    z = bias + sum_j w_j s_j through ks fused multiply-adds: (ks + 2) u (|bias| + sum |w_j s_j|) + sum |w_j| |s_j| (rho_j + u)."""
    B, T, C, ks, w = case["B"], case["T"], case["C"], case["ks"], case["w"]
    y = case["y"].double()
    z, s = convmid_fwd_ref(y, B, T, C, w, case["bias"])
    gate = y[:, C:]
    ds = s.abs() * ((rho_f32(gate) if case["x32"] else rho_fast(gate)) + U)
    absw = w.abs()
    zero = torch.zeros(C)
    mag, _ = convmid_fwd_ref(torch.cat([s.abs(), torch.full_like(s, 40.0)], 1), B, T, C, absw, zero)  # sum |w_j| |s_j| (sigmoid(40) = 1)
    err, _ = convmid_fwd_ref(torch.cat([ds, torch.full_like(s, 40.0)], 1), B, T, C, absw, zero)
    return z, 1.001 * ((ks + 2) * U * (case["bias"].double().abs() + mag) + err) + 2.0 ** -126


SUM_REL = (2.01, 3.01)  # compensated sum of <= 32 terms: 2 u + O(n u^2) of sum |term|; the squares round once more


def conv_sums_bound(z_got, B, T, C):
    """Per-channel sum z and sum z^2 of the partial vectors (added in float64 by the test) against the float64 sums of the z the SAME
    launch stored.  A workgroup adds its <= 32 frames with a compensated (Kahan) sum: 2 u sum |z| and 3 u sum z^2 (SUM_REL)."""
    zd = z_got.double()
    want = torch.cat([zd.sum(0), (zd * zd).sum(0)])
    bound = torch.cat([SUM_REL[0] * U * zd.abs().sum(0), SUM_REL[1] * U * (zd * zd).sum(0)]) * 1.001 + 2.0 ** -126
    return {"want": want, "bound": bound}


def bn_onepass_case(sums_got, z_got, count, C):
    """stats from the partial vectors a forward launch left (sums_got (nparts, 2 C), float32) against the float64 statistics of the z
    it stored: bn_finalize_bound with the partials' own error SUM_REL (the finalize adds and subtracts in double)."""
    nparts = sums_got.shape[0]
    zd = z_got.double()
    exact = torch.cat([zd.sum(0), (zd * zd).sum(0)])[None, :]
    sum_abs = torch.cat([zd.abs().sum(0), (zd * zd).sum(0)])
    rm, rv = torch.zeros(C), torch.ones(C)
    stats, nrm, nrv = bn_finalize_ref(exact, count, C, rm, rv)
    bs, brm, brv = bn_finalize_bound(exact, count, C, rm, rv, sum_rel=SUM_REL, sum_abs=sum_abs)
    return {"nparts": nparts, "C": C, "count": count, "run_mean": rm, "run_var": rv,
            "stats": {"want": stats, "bound": bs}, "rm": {"want": nrm, "bound": brm}, "rv": {"want": nrv, "bound": brv}}


# ---- dropout sites in the GEMM epilogues -------------------------------------------------------------------------------------------
GEMM_M, GEMM_N = 70, 512


def _int_product(m, n, k, seed):
    """Small-integer operands (gemm_cases.int_matrix) whose product is exact in any order of the sums: (a, W, a W^T as float64)."""
    a, w = G.int_matrix(m, k, 0.25, seed), G.int_matrix(n, k, 16.0 / k, seed + 1)
    z = (a.long() @ w.long().t()).double()
    assert float(z.abs().max()) <= 100
    return a, w, z


def dense_act_case(act, backward, p, seed, salt, m=GEMM_M, n=GEMM_N, defect=None):
    """dense_act_drop (forward: u = a W^T + b, h = dropout(act(u))) and dense_act_drop_bwd (du = (dy W2) act'(u) keep / (1 - p)) at
    K = 256, element index mc * N + n.  u is an integer: Swish forward with b = 64 +- 3 (u >= 16, far from 0), otherwise b in
    {-3 .. 3} (ReLU: both signs and zeros).  The product dh of the backward is an integer too, so every ReLU case is exact."""
    a, w, z = _int_product(m, n, 256, 101 + n)
    if backward:
        u = G.int_vector(m * n, -3, 3, 7).view(m, n) if act == ACT_RELU else G.int_vector(m * n, 1, 6, 7).view(m, n)
        ref = z * act_grad_ref(u, act, defect=defect)
        bound = act_bwd_bound(u, z, act, False)
        bias = None
    else:
        bias = G.int_vector(n, -3, 3, 8) + (64.0 if act == ACT_SWISH else 0.0)
        u = (z + bias.double()).float()
        ref, bound = act_fwd_ref(u, act), act_fwd_bound(u, act, False)
    thresh, inv_keep = drop_params(p)
    keep = keep_mask(seed, salt, site_index(m, n, n + 8, defect), p, defect if defect != "mask_index_ld" else None)
    case = {"a": a, "w": w, "bias": bias, "u": u.bfloat16(), "m": m, "n": n, "act": act, "backward": backward, "p": p, "seed": seed,
            "salt": salt, "undropped": ref}
    case.update(_drop_window(ref, bound, keep, inv_keep, torch.bfloat16))
    return case


def dense_act_f32(case, defect=None):
    """float32 restatement of the site on the exact product -> bf16."""
    z = (case["a"].long() @ case["w"].long().t()).float()
    if case["backward"]:
        v = z * act_grad_ref(case["u"].float(), case["act"], dt=torch.float32)
    else:
        v = act_fwd_ref(z + case["bias"], case["act"], dt=torch.float32)
    thresh, inv_keep = drop_params(case["p"])
    m, n = case["m"], case["n"]
    keep = keep_mask(case["seed"], case["salt"], site_index(m, n, n + 8, defect), case["p"], defect if defect != "mask_index_ld" else None)
    if thresh:
        v = torch.where(torch.from_numpy(keep), v * torch.tensor(float(inv_keep)), torch.zeros_like(v))
    return bf16_rne(v)


def dense_join_case(k, p, seed, salt, m=GEMM_M, alpha=0.5, defect=None, with_rs=True):
    """dense_join: out = residual + alpha * dropout(bf16((a W^T + b) * row_scale)), N = 256, element index mc * 256 + n.  Integer
    product and bias, row_scale in {0, 0.5, 1}, residual a multiple of 2^-6, alpha a power of two: `want` is the one float32 value
    fl(residual + alpha * fl(zq * inv_keep)) (alpha * v is exact, with or without a fused multiply-add)."""
    a, w, z = _int_product(m, 256, k, 201 + k)
    bias = G.int_vector(256, -3, 3, 9)
    rs = torch.tensor([1.0, 0.0, 0.5])[torch.randint(0, 3, (m,), generator=_gen(10))]
    rs[0], rs[1] = 0.0, 1.0
    if not with_rs:
        rs = torch.ones(m)
    residual = torch.randint(-512, 512, (m, 256), generator=_gen(11)).float() / 64.0
    zq = ((z + bias.double()) * (1.0 if defect == "row_scale_missing" else rs.double()[:, None])).float()
    assert bool((zq.bfloat16().float() == zq).all())
    thresh, inv_keep = drop_params(p)
    keep = torch.from_numpy(keep_mask(seed, salt, site_index(m, 256, 264, defect), p, defect if defect != "mask_index_ld" else None))
    v = torch.where(keep, zq * torch.tensor(float(inv_keep)) if thresh else zq, torch.zeros_like(zq))
    return {"a": a, "w": w, "bias": bias, "row_scale": rs, "residual": residual, "m": m, "k": k, "alpha": alpha, "p": p, "seed": seed,
            "salt": salt, "want": residual + torch.tensor(alpha) * v}


FFN_HIDDEN = 256  # the smallest hidden size ma_ffn_train_bf16 accepts


def ffn_train_case(p_hidden, p_join, seed, salt_hidden, salt_join, m=GEMM_M, hidden=FFN_HIDDEN, alpha=0.5, defect=None):
    """Both dropout sites of ffn_train and the gk tape: u = a W1^T + b1 an integer >= 16 (b1 = 64 +- 3), h = dropout(swish(u)) at index
    mc * hidden + n, gk = swish'(u) keep / (1 - p) at the same index; x_out = residual + alpha * dropout(bf16(h W2^T + b2)) at index
    mc * 256 + n.  h is a bf16 number >= 16 (a multiple of 2^-3 below 2^10) and W2 holds <= 2 in magnitude: the second product is exact
    in any order, so x_out is computed from the h the SAME launch stored (ffn_join_want)."""
    a, w1, z = _int_product(m, hidden, 256, 301 + hidden)
    b1 = G.int_vector(hidden, -3, 3, 12) + 64.0
    u = (z + b1.double()).float()
    assert float(u.min()) >= 16
    w2 = G.int_matrix(256, hidden, 16.0 / hidden, 302)
    b2 = G.int_vector(256, -3, 3, 13)
    residual = torch.randint(-512, 512, (m, 256), generator=_gen(14)).float() / 64.0
    thresh, inv_keep = drop_params(p_hidden)
    keep = keep_mask(seed, salt_hidden, site_index(m, hidden, hidden + 8, defect), p_hidden, defect if defect != "mask_index_ld" else None)
    case = {"a": a, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "residual": residual, "u": u.bfloat16(), "m": m, "hidden": hidden,
            "alpha": alpha, "p_hidden": p_hidden, "p_join": p_join, "seed": seed, "salt_hidden": salt_hidden, "salt_join": salt_join}
    case["h"] = _drop_window(act_fwd_ref(u, ACT_SWISH), act_fwd_bound(u, ACT_SWISH, False), keep, inv_keep, torch.bfloat16)
    ones = torch.ones_like(u)
    case["gk"] = _drop_window(act_grad_ref(u, ACT_SWISH), act_bwd_bound(u, ones, ACT_SWISH, False), keep, inv_keep, torch.bfloat16)
    return case


def ffn_join_want(case, h_got, defect=None):
    """x_out from the h the launch stored -> {"want": float32}."""
    m = case["m"]
    y = h_got.double().cpu() @ case["w2"].double().t() + case["b2"].double()
    assert bool((y.float().double() == y).all())
    zq = bf16_rne(y.float()).float()
    thresh, inv_keep = drop_params(case["p_join"])
    keep = torch.from_numpy(keep_mask(case["seed"], case["salt_join"], site_index(m, 256, 264, defect), case["p_join"],
                                      defect if defect != "mask_index_ld" else None))
    v = torch.where(keep, zq * torch.tensor(float(inv_keep)) if thresh else zq, torch.zeros_like(zq))
    return {"want": case["residual"] + torch.tensor(case["alpha"]) * v}


# ---- BatchNorm apply + Swish -------------------------------------------------------------------------------------------------------
BN_OUT_CAP = 0.005        # share of bf16 outputs that may differ from the round-to-nearest-even of the float64 value (by one step)
BN_OUT_CAP_F32 = 0.0005   # what the float32 restatement is held to on the same inputs (the CPU self-test)


def bn_swish_fwd_case(rows, C, x32, seed=111):
    """out = swish(gamma (z - mean) rstd + beta) on random z and statistics.  float32: nv = gamma * (z - mean) * rstd + beta rounds four
    times (fewer under contraction): dn = 4 u (|gamma (z - mean) rstd| + |beta|); |swish'| <= 1.1, the sigmoid within rho (fast in the
    bf16 mode, precise in _x32): |out - ref| <= 1.1 dn + |ref| (rho + u).  bf16 outputs: within one bf16 step of ref, and at most
    BN_OUT_CAP of them different from bf16(ref)."""
    g = _gen(seed + rows + C)
    z = torch.randn(rows, C, generator=g) * 2 + 0.5
    stats = torch.cat([0.5 * torch.randn(C, generator=g), 0.3 + torch.rand(C, generator=g)])
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    t = gamma.double() * (z.double() - stats[:C].double()) * stats[C:].double()
    nv = t + beta.double()
    ref = nv * torch.sigmoid(nv)
    dn = 4 * U * (t.abs() + beta.double().abs())
    bound = 1.001 * (1.1 * dn + ref.abs() * ((rho_f32(nv) if x32 else rho_fast(nv)) + U)) + 2.0 ** -126
    return {"z": z, "stats": stats, "gamma": gamma, "beta": beta, "rows": rows, "C": C, "x32": x32, "want": ref, "bound": bound}


def check_bn_swish_out(got, case, cap=BN_OUT_CAP):
    """float32 output: check_bound.  bf16: every element within one bf16 step (plus the float32 bound, which matters only where a
    cancelling sum makes it comparable to the step) of the float64 value and inside the bf16 roundings of ref +- bound; the share that differs from bf16(ref) at most `cap` -> (worst, positions); worst = share / cap for bf16."""
    if case["x32"]:
        return check_bound(got, case)
    got = got.cpu()
    ref = case["want"]
    lo, hi = G.bf16_interval(ref, case["bound"])
    gd = got.double()
    bad = ~((gd >= lo.double()) & (gd <= hi.double())) | ((gd - ref).abs() > G.bf16_step(ref) + case["bound"])
    if bool(bad.any()):
        return math.inf, _positions(bad)
    share = float((G._bits(got.contiguous()) != G._bits(bf16_rne(ref.float()))).float().mean())
    return share / cap, ([("share", share)] if share > cap else [])


def bn_swish_fwd_f32(case):
    z, st, C = case["z"], case["stats"], case["C"]
    nv = case["gamma"] * (z - st[:C]) * st[C:] + case["beta"]
    out = nv * torch.sigmoid(nv)
    return out if case["x32"] else bf16_rne(out)


# ---- training conv module, backward ------------------------------------------------------------------------------------------------
BN_BWD_BLOCKS = 1024      # workgroups of bn_swish_bwd's first stage
BN_BWD_ROWS = (1, 7, 1030)
CONV_BWD_MAX_PARTS = 2048  # kMaxPartBlocks: more strips than this make a convmid_bwd workgroup walk per_block > 1 strips
SUM_DEPTH = 96            # additions a term of the two-stage parameter-gradient sums passes through at most: the rows (strips) of a
#                           workgroup in sequence (<= 32), then partial_reduce / bn_dsum_reduce: <= 2048 / 16 per thread and 16 groups


def _gam(k):
    return k * U / (1 - k * U)


def bn_swish_bwd_ref(dout, z, stats, gamma, beta, dt=torch.float64, defect=None):
    """out = swish(n), n = gamma zhat + beta, zhat = (z - mean) rstd with BATCH statistics ->
    dn = dout swish'(n); dsum = (sum dn | sum dn zhat) = (d_beta | d_gamma); dz = gamma rstd (dn - dsum0 / N - zhat dsum1 / N).
    dsum_not_divided: the two sums enter dz without the 1 / N."""
    C = z.shape[1]
    dout, z, stats, gamma, beta = (t.to(dt) for t in (dout, z, stats, gamma, beta))
    zh = (z - stats[:C]) * stats[C:]
    nv = gamma * zh + beta
    s = torch.sigmoid(nv)
    dn = dout * (s + nv * s * (1 - s))
    s0, s1 = dn.sum(0), (dn * zh).sum(0)
    n = 1.0 if defect == "dsum_not_divided" else float(z.shape[0])
    dz = gamma * stats[C:] * (dn - s0 / n - zh * s1 / n)
    return dn, torch.cat([s0, s1]), dz, {"zh": zh, "nv": nv, "s": s}


def bn_swish_bwd_case(rows, C, x32=False, onehot=None, seed=121, defect=None):
    """Random z, statistics, dout (bf16 values unless x32; onehot: non-zero in that row only) with per-element bounds:
        n: dn_ = 4 u (|gamma zhat| + |beta|);  swish'(n) = s + n s (1 - s), |swish''| <= 0.5:
        d(dn) = |dout| (0.5 dn_ + rho s |1 + n (1 - 2 s)| + 4 u (s + |n| s (1 - s))) + u |dn|
        dsum0: gam(SUM_DEPTH) sum |dn| + sum d(dn);  dsum1: gam(SUM_DEPTH + 1) sum |dn zhat| + sum (d(dn) |zhat| + 2 u |dn zhat|)
        dz = gamma rstd (dn - s0 / N - zhat s1 / N): |gamma rstd| (d(dn) + ds0 / N + |zhat| ds1 / N + 2 u |zhat s1 / N|
             + 4 u (|dn| + |s0 / N| + |zhat s1 / N|)) + 2 u |dz|."""
    g = _gen(seed + rows + C)
    z = torch.randn(rows, C, generator=g) * 2 + 0.5
    stats = torch.cat([0.5 * torch.randn(C, generator=g), 0.3 + torch.rand(C, generator=g)])
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dout = torch.randn(rows, C, generator=g)
    if not x32:
        dout = dout.bfloat16().float()
    if onehot is not None:
        dout = torch.where(torch.arange(rows)[:, None] == onehot, dout, torch.zeros_like(dout))
    dn, dsum, dz, q = bn_swish_bwd_ref(dout, z, stats, gamma, beta, defect=defect)
    if defect is not None:
        return {"dn": {"want": dn}, "dsum": {"want": dsum}, "dz": {"want": dz}}
    zh, nv, s = q["zh"], q["nv"], q["s"]
    rho = rho_f32(nv) if x32 else rho_fast(nv)
    dnv = 4 * U * ((gamma.double() * zh).abs() + beta.double().abs())
    ddn = dout.double().abs() * (0.5 * dnv + rho * s * (1 + nv * (1 - 2 * s)).abs() + 4 * U * (s + nv.abs() * s * (1 - s))) + U * dn.abs()
    ds0 = _gam(SUM_DEPTH) * dn.abs().sum(0) + ddn.sum(0)
    ds1 = _gam(SUM_DEPTH + 1) * (dn * zh).abs().sum(0) + (ddn * zh.abs() + 2 * U * (dn * zh).abs()).sum(0)
    n = float(rows)
    s0, s1 = dsum[:C], dsum[C:]
    gr = (gamma.double() * stats[C:].double()).abs()
    bdz = gr * (ddn + ds0 / n + zh.abs() * ds1 / n + 2 * U * (zh * s1 / n).abs() + 4 * U * (dn.abs() + (s0 / n).abs() + (zh * s1 / n).abs())) \
        + 2 * U * dz.abs()
    f = 1.001
    return {"z": z, "stats": stats, "gamma": gamma, "beta": beta, "dout": dout, "rows": rows, "C": C, "x32": x32, "onehot": onehot,
            "dn": {"want": dn, "bound": f * ddn + 2.0 ** -126}, "dsum": {"want": dsum, "bound": f * torch.cat([ds0, ds1]) + 2.0 ** -126},
            "dz": {"want": dz, "bound": f * bdz + 2.0 ** -126}}


def bn_swish_bwd_f32(case, defect=None):
    dn, dsum, dz, _ = bn_swish_bwd_ref(case["dout"], case["z"], case["stats"], case["gamma"], case["beta"], dt=torch.float32, defect=defect)
    return dn, dsum, dz


def convmid_bwd_ref(dz, y, B, T, C, w, dt=torch.float64, defect=None):
    """Depthwise + GLU backward: ds[t] = sum_j w[c][j] dz[t - (j - pad)] inside the utterance, dy = (ds sig(g) | ds a sig(g) (1 - sig(g))),
    dw[c][j] = sum_t dz[t] s[t + j - pad], db[c] = sum_t dz[t], s = a sig(g) -> (dy (B T, 2 C), dw (C, ks), db (C))."""
    ks = w.shape[1]
    pad = (ks - 1) // 2
    y = y.to(dt).view(B, T, 2 * C)
    a, sg = y[..., :C], torch.sigmoid(y[..., C:])
    s = a * sg
    dzv = dz.to(dt).view(B, T, C).clone()
    wv = w.to(dt).flip(1) if defect == "taps_flipped" else w.to(dt)
    if defect == "last_strip_dropped" and T % 16:
        dzv[:, T // 16 * 16:] = 0  # the frames of the ragged last strip take no part (their dy rows stay unwritten: zero here)
    one = defect == "halo_crosses_utterance"
    dzr, sr = (dzv.reshape(1, B * T, C), s.reshape(1, B * T, C)) if one else (dzv, s)
    n = dzr.shape[1]
    dzp = torch.nn.functional.pad(dzr, (0, 0, pad, pad))
    sp = torch.nn.functional.pad(sr, (0, 0, pad, pad))
    ds = sum(wv[:, j] * dzp[:, 2 * pad - j:2 * pad - j + n] for j in range(ks)).reshape(B, T, C)
    dw = torch.stack([(dzr * sp[:, j:j + n]).sum((0, 1)) for j in range(ks)], 1)
    if defect == "taps_flipped":
        dw = dw.flip(1)
    if defect == "last_strip_dropped" and T % 16:
        ds[:, T // 16 * 16:] = 0
    dy = torch.cat([ds * sg, ds * a * sg * (1 - sg)], -1).reshape(B * T, 2 * C)
    return dy, dw, dzr.sum((0, 1))


def conv_bwd_route_case(ks, T, C, t0, t1, b0=0, b1=0, defect=None):
    """Routing, exact in the float32 mode: dz one-hot (value 2) at (b0, t0) in every channel, s one-hot at (b1, t1): a = 4 there with
    gate = +40 (sigmoid = 1), a = 0 elsewhere with gate = +40; w[c][j] = 2^-(j + c mod 5).  ds has exactly the reversed-tap footprint
    around t0 inside utterance b0 (dy's a half = ds, its gate half = ds a sig (1 - sig) = 0 exactly since 1 - sig = 0);
    d_dw_w[c][t1 - t0 + pad] = 8 when b0 == b1 and the tap exists, every other tap 0; d_dw_b = 2."""
    B = 3
    y = torch.zeros(B, T, 2 * C)
    y[..., C:] = 40.0
    y[b1, t1, :C] = 4.0
    dz = torch.zeros(B, T, C)
    dz[b0, t0] = 2.0
    j = torch.arange(ks, dtype=torch.float64)
    w = torch.exp2(-(j[None, :] + (torch.arange(C) % 5)[:, None].double())).float()
    dy, dw, db = convmid_bwd_ref(dz.view(B * T, C), y.view(B * T, 2 * C), B, T, C, w, defect=defect)
    return {"y": y.view(B * T, 2 * C), "dz": dz.view(B * T, C), "w": w, "B": B, "T": T, "C": C, "ks": ks,
            "dy": {"want": (dy + 0.0).float()}, "dw": {"want": (dw + 0.0).float()}, "db": {"want": db.float()}}


def conv_bwd_random_case(ks, T, C, x32, B=3, seed=131, defect=None, dz=None, dz_bound=None):
    """Random y, dz, w with the bounds of the kernel's arithmetic (rho: the mode's sigmoid):
        ds: (ks + 1) u sum_j |w_j dz|;  a half: dds sg + |ds| sg (rho + 2 u);  gate half = ds (a sg) (1 - sg): dds |a sg (1 - sg)|
            + |ds| (|a| sg (rho + u) (1 - sg) + |a sg| (rho sg + u (1 - sg))) + 2 u |.|
        dw[c][j]: gam(SUM_DEPTH) sum_t |dz s| + sum_t |dz| |s| (rho + u);  db: gam(SUM_DEPTH) sum |dz|."""
    g = _gen(seed + ks + 100 * T + C + B)
    y = torch.randn(B * T, 2 * C, generator=g)
    if not x32:
        y = y.bfloat16().float()
    dzr, w = torch.randn(B * T, C, generator=g), 0.3 * torch.randn(C, ks, generator=g)
    dz = dzr if dz is None else dz  # (given, float64, with its own bound dz_bound: the fused form, whose dz is made in the launch)
    dy, dw, db = convmid_bwd_ref(dz, y, B, T, C, w, defect=defect)
    if defect is not None:
        return {"dy": {"want": dy}, "dw": {"want": dw}, "db": {"want": db}}
    yd = y.double()
    a, gate = yd[:, :C], yd[:, C:]
    sg = torch.sigmoid(gate)
    rho = rho_f32(gate) if x32 else rho_fast(gate)
    ones = torch.cat([torch.ones_like(a), torch.full_like(a, 40.0)], 1)  # a = 1, sigmoid(40) = 1: dy's a half is sum |w| |dz|
    mag, _, _ = convmid_bwd_ref(dz.abs(), ones, B, T, C, w.abs())
    dds = (ks + 1) * U * mag[:, :C]
    if dz_bound is not None:  # the error dz arrives with passes through the same taps
        dds = dds + convmid_bwd_ref(dz_bound, ones, B, T, C, w.abs())[0][:, :C]
    ds = dy[:, :C] / sg
    ba = dds * sg + ds.abs() * sg * (rho + 2 * U)
    bg = dds * (a * sg * (1 - sg)).abs() + ds.abs() * (a.abs() * sg * (rho + U) * (1 - sg) + (a * sg).abs() * (rho * sg + U * (1 - sg))) \
        + 2 * U * dy[:, C:].abs()
    sabs = torch.cat([(a * sg).abs(), torch.full_like(a, 40.0)], 1)
    _, dwm, dbm = convmid_bwd_ref(dz.abs(), sabs, B, T, C, w.abs())
    serr = torch.cat([(a * sg).abs() * (rho + U), torch.full_like(a, 40.0)], 1)
    _, dwe, _ = convmid_bwd_ref(dz.abs(), serr, B, T, C, w.abs())
    if dz_bound is not None:  # ... and into the parameter gradients: sum_t d(dz) |s|, sum_t d(dz)
        _, dwz, dbz = convmid_bwd_ref(dz_bound, sabs, B, T, C, w.abs())
        dwe, dbm = dwe + dwz, dbm + dbz / _gam(SUM_DEPTH)
    f = 1.001
    return {"y": y, "dz": dz, "w": w, "B": B, "T": T, "C": C, "ks": ks, "x32": x32,
            "dy": {"want": dy, "bound": f * torch.cat([ba, bg], 1) + 2.0 ** -126, "x32": x32},
            "dw": {"want": dw, "bound": f * (_gam(SUM_DEPTH) * dwm + dwe) + 2.0 ** -126},
            "db": {"want": db, "bound": f * _gam(SUM_DEPTH) * dbm + 2.0 ** -126}}


def convmid_bwd_f32(case, defect=None):
    dy, dw, db = convmid_bwd_ref(case["dz"], case["y"], case["B"], case["T"], case["C"], case["w"], dt=torch.float32, defect=defect)
    return (dy if case["x32"] else bf16_rne(dy)), dw, db


def check_conv_dy(got, case, cap=BN_OUT_CAP):
    """dy of the conv-module backward: float32 mode check_bound; bf16: both halves (a, gate) separately like check_bn_swish_out."""
    if case["x32"]:
        return check_bound(got, case)
    C = case["want"].shape[1] // 2
    worst, pos = 0.0, []
    for name, sl in (("a", slice(0, C)), ("gate", slice(C, 2 * C))):
        w, p = check_bn_swish_out(got[:, sl], {"x32": False, "want": case["want"][:, sl], "bound": case["bound"][:, sl]}, cap)
        worst = max(worst, w)
        pos += [(name,) + tuple(q) for q in p]
    return worst, pos


def conv_bwd_routes(T):
    """(t0, t1, b0, b1) of the one-hot routing cases: dz at (b0, t0), s at (b1, t1) - the ends, either side of the strip edge 15 | 16,
    the same and different utterances."""
    last = T - 1
    pairs = {(0, 0), (last, last), (0, last), (last, 0), (min(15, last), min(16, last)), (min(16, last), min(15, last)),
             (min(15, last), min(15, last)), (min(16, last), 0)}
    return sorted((t0, t1, 0, 0) for t0, t1 in pairs) + [(last, 0, 0, 1), (0, last, 2, 1), (min(15, last), min(16, last), 1, 2)]


# ---- LayerNorm backward in a GEMM epilogue (dense_lnbwd, ffn_train_bwd) ------------------------------------------------------------
EPI_LN_DEPTH = 24  # a row sum of train_common.h's lnbwd_stats / lnbwd_tail: 16 additions in the lane, 2 shuffles, 3 through LDS, the scaling
SPLITK_K = 1024


def ln_case_from(x, gamma, dy, g0, row_scale, depth=EPI_LN_DEPTH, defect=None):
    """A check_ln_bwd case (accumulating, partials= form) for given rows: dy is what the epilogue's LayerNorm backward consumes."""
    rows, D = x.shape
    zero = torch.zeros(D)
    g, dg, db, _ = ln_bwd_ref(x, gamma, dy, g0, row_scale, True, defect=defect)
    bg, bdg, bdb = ln_bwd_bound(x, gamma, dy, g0, row_scale, True, zero, zero, depth=depth)
    return {"x": x, "gamma": gamma, "dy": dy, "row_scale": row_scale, "g0": g0, "rows": rows, "D": D, "accumulate": True,
            "inplace": False, "onehot": None, "partials": True, "dg0": zero, "db0": zero, "dy_bf16": True,
            "g": {"want": g, "bound": bg}, "dgamma_sum": {"want": dg, "bound": bdg}, "dbeta_sum": {"want": db, "bound": bdb}}


def _ln_rows(m, seed):
    g = _gen(seed)
    x = torch.randn(m, 256, generator=g) * 2 + 0.3
    x[1] = 100.0 + torch.randn(256, generator=g)
    return x, 1 + 0.1 * torch.randn(256, generator=g), torch.randn(m, 256, generator=g)


def dense_lnbwd_case(k=512, m=GEMM_M, defect=None):
    """dense_lnbwd: dy = bf16(a W^T) * row_scale with an integer product (exact), then the LayerNorm backward of ln_case_from and,
    with nxt, dy_next = dropout(g * alpha * row_scale_next) at index mc * 256 + n from the g rows the launch stored (dy_next_case)."""
    a, w, z = _int_product(m, 256, k, 401 + k)
    x, gamma, g0 = _ln_rows(m, 402)
    rs = torch.tensor([1.0, 0.0, 0.5])[torch.randint(0, 3, (m,), generator=_gen(403))]
    rs[0], rs[1], rs[2] = 1.0, 1.0, 0.0
    case = ln_case_from(x, gamma, z.float(), g0, rs, defect=defect)
    case.update({"a": a, "w": w, "k": k, "m": m})
    return case


def ffn_bwd_case(m=GEMM_M, hidden=FFN_HIDDEN):
    """ffn_train_bwd: du = bf16(bf16(dy W2) gk), da = du W1, then the LayerNorm backward on bf16(da).  dy W2 is an integer product;
    gk comes from the tape the forward launch of ffn_train_case wrote (tape_derivative), so du is determined bit for bit by the
    tape - ffn_bwd_want - and the product with W1 is exact (du: bf16 numbers >= 2^-7 apart, W1 small integers, <= 2^12 in sum)."""
    dy, w2t, dh = _int_product(m, hidden, 256, 501)      # dh (m, hidden) = dy (m, 256) . W2 (256, hidden); w2t = W2^T (hidden, 256)
    w1t = G.int_matrix(256, hidden, 16.0 / hidden, 502)  # W1^T (256, hidden): da = du . W1
    x, gamma, g0 = _ln_rows(m, 503)
    return {"dy": dy, "w2t": w2t, "w1t": w1t, "dh": dh, "x": x, "gamma": gamma, "g0": g0, "m": m, "hidden": hidden}


def ffn_bwd_want(case, gk, defect=None):
    """(du bf16, the check_ln_bwd case of the LayerNorm backward behind it) from the tape gk (bf16) the forward stored."""
    du = bf16_rne(case["dh"].float() * gk.float().cpu())
    da = du.double() @ case["w1t"].double().t()
    assert bool((da.float().double() == da).all())
    return du, ln_case_from(case["x"], case["gamma"], bf16_rne(da.float()).float(), case["g0"], None, defect=defect)


# ---- conv1 weight gradient ---------------------------------------------------------------------------------------------------------
# (B, T, idim, C): the 8-channel kernel with LDS staging; the same at C = 512 with 468 positions (64 does not divide them, strips end
# inside a row and inside an utterance); 8-channel WITHOUT staging (the strip's rows would take 48 000 bytes of LDS); the scalar kernel
CONV1_SHAPES = ((2, 31, 80, 256), (3, 9, 80, 512), (1, 5, 2000, 256), (2, 31, 80, 260))


def conv1_dw_ref(dact, x, mean, istd, dt=torch.float64):
    """dw[c][kh 3 + kw] = sum_{b, h1, w1} dact[b, h1, w1, c] xin[b, 2 h1 + kh, 2 w1 + kw], db[c] = sum dact; xin = (x - mean) istd."""
    b, t, idim = x.shape
    h1, w1 = out_hw(t, idim)
    xin = x.to(dt)
    if mean is not None:
        xin = (xin - mean.to(dt)) * istd.to(dt)
    d = dact.to(dt).view(b, h1, w1, -1)
    dw = torch.stack([torch.einsum("bhwc,bhw->c", d, xin[:, kh:kh + 2 * h1 - 1:2, kw:kw + 2 * w1 - 1:2])
                      for kh in range(3) for kw in range(3)], 1)
    return dw, d.sum((0, 1, 2))


def conv1_dw_case(shape, x32, cmvn, seed=141):
    """Integer-valued dact and x in {-2 .. 2} (bf16-exact): without CMVN dw and db are exact integers, added into integer buffers.
    With CMVN (mean in {-1, 0, 1} / 4, istd in [0.5, 1.5)): xin rounds twice (2 u |xin|), every product once, and a term passes through
    at most CONV1_DEPTH additions (a thread's share of the strip, the 8 position groups, then partial_reduce_kernel):
        gam(CONV1_DEPTH) sum |dact xin| + sum |dact| 2 u |xin| + u |dw0 + dw|."""
    b, t, idim, c = shape
    g = _gen(seed + idim + c)
    h1, w1 = out_hw(t, idim)
    x = torch.randint(-2, 3, (b, t, idim), generator=g).float()
    dact = torch.randint(-2, 3, (b * h1 * w1, c), generator=g).float()
    mean = istd = None
    if cmvn:
        mean, istd = torch.randint(-1, 2, (idim,), generator=g).float() / 4, 0.5 + torch.rand(idim, generator=g)
    dw0, db0 = torch.randint(-8, 9, (c, 9), generator=g).float(), torch.randint(-8, 9, (c,), generator=g).float()
    dw, db = conv1_dw_ref(dact, x, mean, istd)
    case = {"shape": shape, "x32": x32, "x": x, "dact": dact if x32 else dact.bfloat16(), "mean": mean, "istd": istd, "dw0": dw0, "db0": db0}
    if not cmvn:
        case["dw"] = {"want": (dw0.double() + dw).float()}
        case["db"] = {"want": (db0.double() + db).float()}
        return case
    xin_abs = ((x.double() - mean.double()) * istd.double()).abs()
    mag, _ = conv1_dw_ref(dact.abs(), xin_abs, None, None)
    bound = 1.001 * (_gam(CONV1_DEPTH) * mag + 2 * U * mag + U * (dw0.double() + dw).abs()) + 2.0 ** -126
    case["dw"] = {"want": dw0.double() + dw, "bound": bound}
    case["db"] = {"want": (db0.double() + db).float()}  # db does not see the CMVN: exact
    return case


CONV1_DEPTH = 160


def check_conv1_dw(got, case):
    worst, pos = 0.0, []
    for name, t in zip(("dw", "db"), got):
        w, p = (check_bound if "bound" in case[name] else check_exact)(t.cpu(), case[name])
        worst = max(worst, w)
        pos += [(name,) + tuple(q) for q in p]
    return worst, pos


def conv1_dw_f32(case, transposed=False):
    """float32 restatement; transposed: the taps read as (kw, kh) - a mistake the check must catch."""
    dw, db = conv1_dw_ref(case["dact"].float(), case["x"], case["mean"], case["istd"], dt=torch.float32)
    if transposed:
        dw = dw.view(-1, 3, 3).transpose(1, 2).reshape(-1, 9)
    return case["dw0"] + dw, case["db0"] + db
