"""The float64 NumPy restatement of DeepSpeech2's convolution front end (MaskConv) in TRAINING mode, in the reference's layouts
(x (B, 1, F, T), weights (out, in, kf, kt), activations (B, 32, F', T1)), that test_ds2_frontend_train_cases_cpu.py checks against
torch.autograd and the GPU tests measure the device against.  Built on deepspeech2_cases.conv2d.

  forward   y1 = conv1(x); per channel over (B, F1, T1): mean, BIASED variance; a1 = tanh(gamma (y1 - mean) / sqrt(var + 1e-5) + beta);
            y2 = conv2(a1), the same again -> a2 (B, 32, F2, T1).  moving = 0.9 moving + 0.1 (mean, UNBIASED variance).
  backward  closed form: dn = da (1 - a^2), d_beta = sum dn, d_gamma = sum dn xhat, dz = gamma rstd (dn - mean dn - xhat mean(dn xhat)),
            then the convolution's weight and input gradients.
  rounding-only   the same float64 arithmetic with bf16 at exactly the device's points: act1 (conv2's input, in both directions), conv2's
            weights (in both directions), xin (the output), the dz2 image.  tanh' is taken on the UNROUNDED activation, as the device
            recomputes it from the raw float32 convolution output.  dz1 stays float32 on the device: not rounded here.
S = relrms(rounding-only, exact) per parameter is the yardstick; the device is allowed 2 S (deepspeech2_cases has the reasoning).
No figure here is measured on the code under test."""
import functools

import numpy as np
import torch

import deepspeech2_cases as C

BN_EPS, MOMENTUM = 1e-5, 0.1
PARAMS = ("conv.conv1.weight", "conv.bn1.gamma", "conv.bn1.beta", "conv.conv2.weight", "conv.bn2.gamma", "conv.bn2.beta")
DEFECTS = ("stats_constant", "xhat_term_dropped", "taps_not_reversed", "parity_swapped", "unbiased_normalise", "row22_kept")
U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, np.float64)


# ---- convolution backward -----------------------------------------------------------------------------------------------------------------
def conv2d_backward(x, w, dy, stride, pad):
    """The gradients of deepspeech2_cases.conv2d: -> (dx like x, dw like w)."""
    B, Cin, F, T = x.shape
    _, _, kf, kt = w.shape
    (sf, st), (pf, pt) = stride, pad
    Fo, To = dy.shape[2], dy.shape[3]
    xp = np.zeros((B, Cin, F + 2 * pf, T + 2 * pt))
    xp[:, :, pf:pf + F, pt:pt + T] = x
    dxp, dw = np.zeros_like(xp), np.zeros(w.shape)
    for a in range(kf):
        for b in range(kt):
            sl = (slice(None), slice(None), slice(a, a + sf * (Fo - 1) + 1, sf), slice(b, b + st * (To - 1) + 1, st))
            dw[:, :, a, b] = np.einsum("boft,bcft->oc", dy, xp[sl])
            dxp[sl] += np.einsum("oc,boft->bcft", w[:, :, a, b], dy)
    return dxp[:, :, pf:pf + F, pt:pt + T], dw


# ---- the device's forms of conv2's two gradients (frequency rows of the operand images), with their planted defects -----------------------
def conv2_dw_by_rows(dz2, act1, keep_row22=False):
    """conv2's weight gradient as the device forms it: per time tap j and output frequency fo the product of dz2[:, :, fo] with the 22
    padded input rows 2 fo .. 2 fo + 21 of act1 shifted by j - 5 frames, accumulated over fo into (11, 32, 22, 32) [j, co, row, ci]; the
    22nd row is padding of the operand and is dropped.  keep_row22 (a defect): rows 1 .. 21 are kept instead of 0 .. 20."""
    B, _, F1, T1 = act1.shape
    F2 = dz2.shape[2]
    ap = np.zeros((B, 32, 2 * (F2 - 1) + 22, T1 + 10))
    ap[:, :, 10:10 + F1, 5:5 + T1] = act1
    acc = np.zeros((11, 32, 22, 32))
    for j in range(11):
        for fo in range(F2):
            acc[j] += np.einsum("bot,bcrt->orc", dz2[:, :, fo, :], ap[:, :, 2 * fo:2 * fo + 22, j:j + T1])
    rows = acc[:, :, 1:22, :] if keep_row22 else acc[:, :, :21, :]
    return rows.transpose(1, 3, 2, 0)  # (co, ci, df, j)


def conv2_dx_by_rows(dz2, w2, F1, reverse_taps=True, swap_parity=False):
    """conv2's input gradient as the device forms it: for the padded input row r = fi + 10 with parity p the 12 output rows
    fo = (r - p) / 2 - 10 + k, k = 0 .. 11, of the zero-padded dz2 against W_p[k] = w2[:, :, p + 2 (10 - k), :] (zero where that tap does
    not exist), the 11 time taps reversed.  Defects: the taps not reversed; the two parity images swapped."""
    B, _, F2, T1 = dz2.shape
    img = np.zeros((2, 12, 32, 32, 11))  # [p, k, co, ci, j]
    for p in (0, 1):
        for k in range(11):
            if p + 2 * (10 - k) <= 20:
                img[p, k] = w2[:, :, p + 2 * (10 - k), :]
    zp = np.zeros((B, 32, F2 + 11, T1 + 10))
    zp[:, :, 5:5 + F2, 5:5 + T1] = dz2
    dx = np.zeros((B, 32, F1, T1))
    for fi in range(F1):
        r = fi + 10
        p = r & 1
        q0 = (r - p) // 2 - 10 + 5
        wimg = img[1 - p if swap_parity else p]
        for j in range(11):  # forward: y2[t] reads act1[t + j - 5], so act1[t'] collects dz2[t' - (j - 5)]
            shift = (10 - j) if reverse_taps else j
            dx[:, :, fi, :] += np.einsum("bkot,koc->bct", zp[:, :, q0:q0 + 12, shift:shift + T1].transpose(0, 2, 1, 3), wimg[:, :, :, j])
    return dx


# ---- train-mode MaskConv ----------------------------------------------------------------------------------------------------------------------
def _bn_tanh(y, gamma, beta, unbiased_normalise=False):
    n = y.size // y.shape[1]
    mean = y.mean((0, 2, 3))
    var = ((y - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
    vn = var * n / (n - 1) if unbiased_normalise else var
    rstd = 1.0 / np.sqrt(vn + BN_EPS)
    xhat = (y - mean[None, :, None, None]) * rstd[None, :, None, None]
    a = np.tanh(_f64(gamma)[None, :, None, None] * xhat + _f64(beta)[None, :, None, None])
    return dict(mean=mean, var=var, unbiased=var * n / (n - 1), rstd=rstd, xhat=xhat, a=a, n=n)


def forward(p, x, rounding=False, defect=None):
    """-> dict: y1, bn1 (mean, var, unbiased, rstd, xhat, a), act1 (conv2's input: a1, rounded in the rounding-only form), y2, bn2, out
    (B, 32, F2, T1) (a2, rounded in the rounding-only form), moving {name: new value}."""
    assert defect is None or defect in DEFECTS
    r = C.bf16_round if rounding else _f64
    ub = defect == "unbiased_normalise"
    w1, w2 = _f64(p["conv.conv1.weight"]), r(_f64(p["conv.conv2.weight"]))
    y1 = C.conv2d(_f64(x), w1, (2, 2), (20, 5))
    bn1 = _bn_tanh(y1, p["conv.bn1.gamma"], p["conv.bn1.beta"], ub)
    act1 = r(bn1["a"])
    y2 = C.conv2d(act1, w2, (2, 1), (10, 5))
    bn2 = _bn_tanh(y2, p["conv.bn2.gamma"], p["conv.bn2.beta"], ub)
    moving = {}
    for i, bn in ((1, bn1), (2, bn2)):
        moving["conv.bn%d.moving_mean" % i] = (1 - MOMENTUM) * _f64(p["conv.bn%d.moving_mean" % i]) + MOMENTUM * bn["mean"]
        moving["conv.bn%d.moving_variance" % i] = (1 - MOMENTUM) * _f64(p["conv.bn%d.moving_variance" % i]) + MOMENTUM * bn["unbiased"]
    return dict(x=_f64(x), w2=w2, y1=y1, bn1=bn1, act1=act1, y2=y2, bn2=bn2, out=r(bn2["a"]), moving=moving, rounding=rounding)


def _bn_tanh_backward(bn, gamma, da, defect=None):
    dn = da * (1.0 - bn["a"] ** 2)
    d_beta, d_gamma = dn.sum((0, 2, 3)), (dn * bn["xhat"]).sum((0, 2, 3))
    g = (_f64(gamma) * bn["rstd"])[None, :, None, None]
    if defect == "stats_constant":
        return g * dn, d_gamma, d_beta
    m1 = (d_beta / bn["n"])[None, :, None, None]
    m2 = 0.0 if defect == "xhat_term_dropped" else (d_gamma / bn["n"])[None, :, None, None]
    return g * (dn - m1 - bn["xhat"] * m2), d_gamma, d_beta


def backward(p, fwd, dout, defect=None):
    """dout (B, 32, F2, T1) = d loss / d out -> {the six gradients, "dz1", "dz2", "dact1"}; rounding as `fwd` was computed.  With a
    defect the device's row forms of conv2's gradients are used (they equal the closed forms without one: the CPU test checks it)."""
    assert defect is None or defect in DEFECTS
    r = C.bf16_round if fwd["rounding"] else _f64
    g = {}
    dz2, g["conv.bn2.gamma"], g["conv.bn2.beta"] = _bn_tanh_backward(fwd["bn2"], p["conv.bn2.gamma"], _f64(dout), defect)
    dz2 = r(dz2)
    F1 = fwd["act1"].shape[2]
    if defect in ("taps_not_reversed", "parity_swapped", "row22_kept"):
        dact1 = conv2_dx_by_rows(dz2, fwd["w2"], F1, reverse_taps=defect != "taps_not_reversed", swap_parity=defect == "parity_swapped")
        g["conv.conv2.weight"] = conv2_dw_by_rows(dz2, fwd["act1"], keep_row22=defect == "row22_kept")
    else:
        dact1, g["conv.conv2.weight"] = conv2d_backward(fwd["act1"], fwd["w2"], dz2, (2, 1), (10, 5))
    dz1, g["conv.bn1.gamma"], g["conv.bn1.beta"] = _bn_tanh_backward(fwd["bn1"], p["conv.bn1.gamma"], dact1, defect)
    _, g["conv.conv1.weight"] = conv2d_backward(fwd["x"], _f64(p["conv.conv1.weight"]), dz1, (2, 2), (20, 5))
    g.update(dz1=dz1, dz2=dz2, dact1=dact1)
    return g


def conv1_dw_abs_terms(x, dz1):
    """sum over (b, f1, t1) of |dz1 x| per output (32, 1, 41, 11): the scale of conv1's weight-gradient accumulation bound."""
    return conv2d_backward(np.abs(_f64(x)), np.zeros((32, 1, 41, 11)), np.abs(_f64(dz1)), (2, 2), (20, 5))[1]


# ---- torch.autograd, the independent yardstick -------------------------------------------------------------------------------------------------
def autograd_frontend(p, x):
    """float64 torch: -> ({name: leaf tensor}, out (B, 32, F2, T1) with its graph, {name: new moving statistic})"""
    import torch.nn.functional as F

    leaves = {n: torch.tensor(_f64(p[n]), dtype=torch.float64, requires_grad=True) for n in PARAMS}
    h = torch.tensor(_f64(x), dtype=torch.float64)
    moving = {}
    for i, (stride, pad) in ((1, ((2, 2), (20, 5))), (2, ((2, 1), (10, 5)))):
        h = F.conv2d(h, leaves["conv.conv%d.weight" % i], stride=stride, padding=pad)
        rm = torch.tensor(_f64(p["conv.bn%d.moving_mean" % i]))
        rv = torch.tensor(_f64(p["conv.bn%d.moving_variance" % i]))
        h = torch.tanh(F.batch_norm(h, rm, rv, leaves["conv.bn%d.gamma" % i], leaves["conv.bn%d.beta" % i], training=True,
                                    momentum=MOMENTUM, eps=BN_EPS))
        moving["conv.bn%d.moving_mean" % i], moving["conv.bn%d.moving_variance" % i] = rm.numpy(), rv.numpy()
    return leaves, h, moving


def autograd(p, x, dout):
    """-> (out, {name: gradient}, moving) of sum(out * dout)"""
    leaves, out, moving = autograd_frontend(p, x)
    (out * torch.tensor(_f64(dout))).sum().backward()
    return out.detach().numpy(), {n: v.grad.numpy() for n, v in leaves.items()}, moving


# ---- layouts of the device ------------------------------------------------------------------------------------------------------------------------
def to_device_xin(a, Kpad):
    """(B, 32, F2, T1) -> (T1, B, Kpad), feature f * 32 + c, the padding columns zero."""
    B, Cc, F2, T1 = a.shape
    out = np.zeros((T1, B, Kpad))
    out[:, :, :Cc * F2] = a.transpose(3, 0, 2, 1).reshape(T1, B, F2 * Cc)
    return out


def from_device_xin(a, F2):
    """(T1, B, >= F2 * 32) with feature f * 32 + c -> (B, 32, F2, T1)"""
    T1, B, _ = a.shape
    return _f64(a)[:, :, :F2 * 32].reshape(T1, B, F2, 32).transpose(1, 3, 2, 0)


def from_channel_last(a):
    """(T1, B, F', 32) -> (B, 32, F', T1)"""
    return _f64(a).transpose(1, 3, 2, 0)


def to_channel_last(a):
    """(B, 32, F', T1) -> (T1, B, F', 32)"""
    return np.ascontiguousarray(_f64(a).transpose(3, 0, 2, 1))


def make_dout(cfg, seed, scale=1.0):
    """A random d loss / d out (B, 32, F2, T1), unit normal times `scale`, of float32 values (the device takes it as float32)."""
    F = C.n_freq(cfg["sample_rate"], cfg["window_size"])
    F2 = C.conv_out(C.conv_out(F, 41, 20, 2), 21, 10, 2)
    T1 = C.conv_out(cfg["T"], 11, 5, 2)
    return np.random.RandomState(seed).normal(0.0, scale, (cfg["B"], 32, F2, T1)).astype(np.float32).astype(np.float64)


def yardstick(p, x, dout):
    """-> (exact gradients, rounding-only gradients, {name: S}, exact forward, rounding-only forward)"""
    fe, fr = forward(p, x), forward(p, x, rounding=True)
    ge, gr = backward(p, fe, dout), backward(p, fr, dout)
    return ge, gr, {n: C.relrms(gr[n], ge[n]) for n in PARAMS}, fe, fr


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """(cfg, state, x, dout, exact gradients, rounding-only gradients, S, exact forward, rounding-only forward) of SMALL /
    YAML_GEOMETRY with the weights and input of deepspeech2_cases.model_case, computed once per process and left unchanged."""
    cfg = {"small": C.SMALL, "yaml-geometry": C.YAML_GEOMETRY}[name]
    state, x = C.make_state(cfg, 11 + seed), C.make_input(cfg, 12 + seed, pad_frames=6)
    dout = make_dout(cfg, 13 + seed)
    return (cfg, state, x, dout) + yardstick(state, x, dout)


def cosine(a, b):
    a, b = _f64(a).ravel(), _f64(b).ravel()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def stats_failures(mean, var, y, channel_axis):
    """The GPU statistics comparator: (mean, biased variance) per channel against the float64 moments of y itself.
    |mean - mean64| <= 4 u mean|y| and |var - var64| <= 12 u E[y^2]: double partials leave 2 u on each sum, one rounding on store,
    var = E[y^2] - mean^2 and mean|y|^2 <= E[y^2].  -> a list of failure strings."""
    y = np.moveaxis(_f64(y), channel_axis, 0).reshape(32, -1)
    m64, q64, a64 = y.mean(1), (y * y).mean(1), np.abs(y).mean(1)
    v64 = ((y - m64[:, None]) ** 2).mean(1)
    out = []
    for c in range(32):
        if not abs(mean[c] - m64[c]) <= 4 * U * a64[c]:
            out.append("mean[%d]: %.9g against %.9g" % (c, mean[c], m64[c]))
        if not abs(var[c] - v64[c]) <= 12 * U * q64[c]:
            out.append("var[%d]: %.9g against %.9g" % (c, var[c], v64[c]))
    return out
