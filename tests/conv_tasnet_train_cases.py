"""The CPU reference side of Conv-TasNet training (test_conv_tasnet_train_cpu.py / test_conv_tasnet_train_gpu.py): the network of
conv_tasnet_cases.forward restated over a dtype and a 1 x 1 convolution, Convtasnet_Loss with the length mask, gradients by
torch.autograd in three forms, the closed-form SI-SNR gradient and gLN backward, nn.SGD, the cases and the comparators.

  form "a": exact float64.
  form "b": float32 throughout - the same code on .float() tensors.
  form "c": float64 with every 1 x 1 convolution's operands rounded to bf16 in the forward AND in the backward (dY and the saved
            operands, where the device rounds: dX = bf16(dY) . bf16(W), dW = bf16(dY)^T . bf16(X)).

Nothing here imports the code under test, and no figure here is measured on it."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_tasnet_cases as C

EPS = 1e-8
TINY = dict(N=64, L=20, B=64, H=128, P=3, X=8, R=1, C=2)
S_CEILING_GRAD = 0.2   # a changed restatement cannot widen its own tolerance past this (0.13 measured for conv1x1 at SMALL)
COS_MIN = 0.98
MARGIN = 4.0           # float32 tests: x the float32 restatement's own error (summation order)


def samples(K, L=20):
    return (K + 1) * (L // 2)  # T with (T - L) // (L / 2) + 1 == K and an estimate of the same length


class _Bf16Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        xr, wr = C.bf16_round(x), C.bf16_round(w)
        ctx.save_for_backward(xr, wr)
        return F.conv1d(xr, wr)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = C.bf16_round(dy)
        return torch.einsum("mok,oi->mik", dyr, wr[:, :, 0]), torch.einsum("mok,mik->oi", dyr, xr)[:, :, None]


def gln(y):
    mean = y.mean(dim=(1, 2), keepdim=True)
    var = (y - mean).pow(2).mean(dim=(1, 2), keepdim=True)
    return (y - mean) / torch.sqrt(var + EPS)


def dwconv(t, w, d, defect=None):
    H = w.shape[0]
    if defect == "tap":  # a dropped tap
        w = w * torch.tensor([1.0, 1.0, 0.0], dtype=w.dtype)
    return F.conv1d(t, w, padding=d, dilation=d, groups=H)


def forward(w, cfg, mixture, overlap="paired", conv=F.conv1d, defect=None, sites=None):
    """conv_tasnet_cases.forward on the tensors of `w` as they are (their dtype, their autograd state).  `sites`: a list that
    receives the input of every ReLU / PReLU (the encoder output, each conv1x1 and depthwise output, the mask scores)."""
    keep = (lambda t: sites.append(t.detach())) if sites is not None else (lambda t: None)
    N, L, H, X, R, Cs = (cfg[k] for k in ("N", "L", "H", "X", "R", "C"))
    x = mixture
    M = x.shape[0]
    enc = F.conv1d(x[:, None, :], w["encoder.conv1d_U.weight"], stride=L // 2)
    keep(enc)
    mixture_w = F.relu(enc)
    K = mixture_w.shape[2]
    y = conv(gln(mixture_w), w["separator.bottleneck_conv1x1.weight"])
    for r in range(R):
        for xi in range(X):
            p = "separator.temporal_conv_net.%d.%d." % (r, xi)
            t = conv(y, w[p + "conv1x1.weight"])
            keep(t)
            t = gln(F.prelu(t, w[p + "prelu.weight"]))
            t = dwconv(t, w[p + "dsconv.depthwise_conv.weight"], 2 ** xi, defect)
            keep(t)
            t = F.prelu(t, w[p + "dsconv.prelu.weight"])
            t = _GlnNoCross.apply(t) if defect == "gln" else gln(t)
            t = conv(t, w[p + "dsconv.pointwise_conv.weight"])
            y = _DropResidualGrad.apply(y, t) if defect == "residual" else y + t
    score = conv(y, w["separator.mask_conv1x1.weight"]).view(M, Cs, N, K)
    keep(score)
    source_w = (mixture_w[:, None] * F.relu(score)).transpose(2, 3)
    frames = source_w @ w["decoder.basis_signals.weight"].t()
    return C.overlap_paired(frames) if overlap == "paired" else C.overlap_true(frames)


class _GlnNoCross(torch.autograd.Function):
    """gLN whose backward lacks the mean(dy * xhat) term (a planted defect for the comparator proof)."""

    @staticmethod
    def forward(ctx, y):
        mean = y.mean(dim=(1, 2), keepdim=True)
        rstd = 1.0 / torch.sqrt((y - mean).pow(2).mean(dim=(1, 2), keepdim=True) + EPS)
        ctx.save_for_backward(rstd)
        return (y - mean) * rstd

    @staticmethod
    def backward(ctx, dy):
        (rstd,) = ctx.saved_tensors
        return (dy - dy.mean(dim=(1, 2), keepdim=True)) * rstd


class _DropResidualGrad(torch.autograd.Function):
    """y + t whose backward sends nothing along y (a missing residual term)."""

    @staticmethod
    def forward(ctx, y, t):
        return y + t

    @staticmethod
    def backward(ctx, d):
        return torch.zeros_like(d), d


def si_snr_table(source, estimate, lengths, mask_tail=True):
    """separation_loss.py:188-216 as differentiable torch ops, masked by the lengths: [b, i_est, j_target]."""
    B, Cs, T = source.shape
    rows = []
    for b in range(B):
        n = int(lengths[b]) if mask_tail else T
        e, t = estimate[b, :, :n], source[b, :, :n]
        den = float(int(lengths[b]))
        e, t = e - e.sum(1, keepdim=True) / den, t - t.sum(1, keepdim=True) / den
        e, t = e[:, None, :], t[None, :, :]
        proj = (e * t).sum(2, keepdim=True) * t / ((t ** 2).sum(2, keepdim=True) + EPS)
        noise = e - proj
        rows.append(10.0 * torch.log((proj ** 2).sum(2) / ((noise ** 2).sum(2) + EPS) + EPS) / math.log(10.0))
    return torch.stack(rows)


def pit_loss(source, estimate, lengths, mask_tail=True):
    """Convtasnet_Loss: (loss, perms, table); the first permutation wins a tie."""
    table = si_snr_table(source, estimate, lengths, mask_tail)
    B, Cs, _ = table.shape
    total, perms = 0.0, []
    for b in range(B):
        perm, _ = C.best_permutation(table[b].detach().double().numpy())
        perms.append(perm)
        total = total + sum(table[b, perm[j], j] for j in range(Cs)) / Cs
    return -total / B, perms, table


_FORMS = {"a": (torch.float64, F.conv1d), "b": (torch.float32, F.conv1d), "c": (torch.float64, _Bf16Conv.apply)}


def loss(state, cfg, mixture, sources, lengths, overlap="paired", form="a"):
    dtype, conv = _FORMS[form]
    w = {k: v.to(dtype) for k, v in state.items()}
    est = forward(w, cfg, mixture.to(dtype), overlap, conv)
    return float(pit_loss(sources.to(dtype), est, lengths)[0])


def grads(state, cfg, mixture, sources, lengths, overlap="paired", form="a", defect=None):
    """(loss, {name: gradient}, {"estimate": d loss / d estimate}) by torch.autograd."""
    dtype, conv = _FORMS[form]
    w = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    est = forward(w, cfg, mixture.to(dtype), overlap, conv, defect)
    est.retain_grad()
    value, _, _ = pit_loss(sources.to(dtype), est, lengths, mask_tail=defect != "tail")
    value.backward()
    return float(value.detach()), {k: v.grad.detach() for k, v in w.items()}, {"estimate": est.grad.detach()}


def si_snr_grad_closed(source, estimate, lengths, perms):
    """d(-mean_b(sum_j snr[b, perm_j, j] / C)) / d estimate in closed float64 form (NumPy); 0 at and beyond the length."""
    source, estimate = np.asarray(source, np.float64), np.asarray(estimate, np.float64)
    B, Cs, T = source.shape
    out = np.zeros_like(estimate)
    for b in range(B):
        n = int(lengths[b])
        for j in range(Cs):
            i = perms[b][j]
            a, r = estimate[b, i, :n], source[b, j, :n]
            a, r = a - a.sum() / n, r - r.sum() / n
            dot, S = np.sum(a * r), np.sum(r * r)
            en = S + EPS
            noise = a - dot * r / en
            pp, nn, nr = dot * dot * S / (en * en), np.sum(noise * noise), np.sum(noise * r)
            q = pp / (nn + EPS)
            k = 10.0 / (math.log(10.0) * (q + EPS)) * (-1.0 / (B * Cs))
            dpp, dnn = k / (nn + EPS), -k * pp / (nn + EPS) ** 2
            g = (dpp * 2 * dot * S / (en * en) - dnn * 2 * nr / en) * r + dnn * 2 * noise
            out[b, i, :n] = g - g.sum() / n
    return out


def gln_bwd_closed(y, dy):
    """dx = (dy - mean(dy) - xhat mean(dy xhat)) / sigma per utterance, on (M, channels, K) float64 tensors."""
    mean = y.mean(dim=(1, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt((y - mean).pow(2).mean(dim=(1, 2), keepdim=True) + EPS)
    xhat = (y - mean) * rstd
    return (dy - dy.mean(dim=(1, 2), keepdim=True) - xhat * (dy * xhat).mean(dim=(1, 2), keepdim=True)) * rstd


def sgd_step(params, grads_, bufs, lr, momentum, weight_decay):
    """nn.SGD(momentum, weight_decay) of train.py:91-96 restated: in place on dicts of tensors; bufs is {} before the first step."""
    for k, p in params.items():
        g = grads_[k] + weight_decay * p
        if momentum > 0:
            bufs[k] = g.clone() if k not in bufs else momentum * bufs[k] + g
            g = bufs[k]
        p -= lr * g


def trajectory(state, cfg, mixture, sources, lengths, overlap, form, steps, lr, momentum, weight_decay):
    """The losses BEFORE each of `steps` SGD steps on one batch, and the loss after the last, in the form's arithmetic."""
    dtype = _FORMS[form][0]
    params, bufs, out = {k: v.detach().to(dtype).clone() for k, v in state.items()}, {}, []
    for _ in range(steps):
        value, g, _ = grads(params, cfg, mixture, sources, lengths, overlap, form)
        out.append(value)
        sgd_step(params, g, bufs, lr, momentum, weight_decay)
    out.append(loss(params, cfg, mixture, sources, lengths, overlap, form))
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
#        name     K    R  overlap   short  swapped
CASES = {"k150": (150, 1, "paired", 0, False),    # above the largest dilation; three 64-row tiles, the last ragged
         "k100": (100, 1, "paired", 0, False),    # dilation 128 exceeds the utterance: its outer taps never land
         "k64": (64, 1, "paired", 0, False),      # exactly one tile
         "ragged": (150, 1, "paired", 137, False),
         "true": (100, 1, "true", 0, False),
         "r2": (64, 2, "paired", 0, False),
         "swap": (64, 1, "paired", 0, True)}
M = 2
_made = {}


FLIP_GUARD = 8.0


def flip_margin(state, cfg, mixture, overlap):
    """How far the inputs of the ReLU / PReLU masks stay from zero, in units of FLIP_GUARD x the float32 error there: the smallest
    |v_a| / (FLIP_GUARD max(|v_b - v_a|, rms(v_b - v_a) of that tensor)) over every element v of every mask input, v_a from the
    float64 forward and v_b from the float32 one.  A mask is a discrete choice, like the permutation: where an input lies within
    float32 rounding of zero, two correct float32 evaluations may take different sides, and ONE flipped element moves a gradient tensor
    by about 1 / sqrt(its elements) - 6e-3 here, a thousand times the float32 tolerance - which says nothing about the kernels.  The
    float32 cases are therefore drawn so that this margin is at least 1 (asserted on the CPU), from the reference alone."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        sites = []
        with torch.no_grad():
            forward({k: v.to(dtype) for k, v in state.items()}, cfg, mixture.to(dtype), overlap, sites=sites)
        out[dtype] = [t.double() for t in sites]
    worst = float("inf")
    for a, b in zip(out[torch.float64], out[torch.float32]):
        err = (b - a).abs()
        guard = FLIP_GUARD * torch.maximum(err, err.pow(2).mean().sqrt())
        worst = min(worst, float((a.abs() / guard).min()))
    return worst


def case(name):
    """dict(cfg, state, mixture, sources, lengths, overlap, perms): built once and shared; nobody changes it.

    The mixture is the first of the seeds 5 + K, 1005 + K, ... whose flip_margin is at least 1.

    The targets are the form (a) estimate of the untrained network - in the order wanted - plus noise of its own rms, so that the
    wanted permutation wins by far more than 1 dB and no form or device can choose another one."""
    if name in _made:
        return _made[name]
    K, R, overlap, short, swapped = CASES[name]
    cfg = dict(TINY, R=R)
    T = samples(K)
    state = C.make_state(cfg, 11 + R)
    for attempt in range(64):
        mixture = C.make_mixture(M, T, 5 + K + 1000 * attempt)
        if flip_margin(state, cfg, mixture, overlap) >= 1.0:
            break
    else:
        raise AssertionError("no mixture seed keeps the masks clear of zero")
    with torch.no_grad():
        est = forward({k: v.double() for k, v in state.items()}, cfg, mixture.double(), overlap)
    g = torch.Generator().manual_seed(K + R)
    order = [1, 0] if swapped else [0, 1]
    sources = (est[:, order] + est.pow(2).mean(dim=2, keepdim=True).sqrt() * torch.randn(est.shape, generator=g, dtype=torch.float64)).float()
    lengths = [T, T - short]
    _made[name] = dict(cfg=cfg, state=state, mixture=mixture, sources=sources, lengths=lengths, overlap=overlap,
                       want_perm=tuple(order), K=K, T=T, attempt=attempt)
    return _made[name]


_ref = {}


def reference(name, form):
    """grads() of a case in a form, computed once."""
    key = (name, form)
    if key not in _ref:
        c = case(name)
        _ref[key] = grads(c["state"], c["cfg"], c["mixture"], c["sources"], c["lengths"], c["overlap"], form)
    return _ref[key]


# ---- comparators ------------------------------------------------------------------------------------------------------------------------
def groups(g):
    """{tensor name: flat float64 vector}, the 1-element PReLU slopes gathered into ONE vector."""
    out, slopes = {}, []
    for k in sorted(g):
        v = torch.as_tensor(g[k]).detach().double().cpu().reshape(-1)
        if k.endswith("prelu.weight"):
            slopes.append(v)
        else:
            out[k] = v
    out["prelu"] = torch.cat(slopes)
    return out


def kind(name):
    """The parameter group of a tensor (bf16 mode compares per group)."""
    for key in ("conv1d_U", "bottleneck", "depthwise", "pointwise", "mask_conv1x1", "basis_signals", "conv1x1", "prelu"):
        if key in name:
            return key
    raise KeyError(name)


def by_kind(g):
    out = {}
    for k, v in groups(g).items():
        out.setdefault(kind(k), []).append(v)
    return {k: torch.cat(v) for k, v in out.items()}


def check_f32(got, a, b):
    """Every tensor of `got` within MARGIN x relrms(b, a) of (a); returns the list of failures (name, got, allowed)."""
    G, A, Bf = groups(got), groups(a), groups(b)
    bad = []
    for k in A:
        allowed = MARGIN * C.relrms(Bf[k], A[k])
        err = C.relrms(G[k], A[k])
        if not err <= allowed:
            bad.append((k, err, allowed))
    return bad


def check_bf16(got, a, c):
    """Per parameter group relrms(got, a) <= 2 S, S = relrms(c, a) <= S_CEILING_GRAD, and the cosine over all parameters."""
    G, A, Cc = by_kind(got), by_kind(a), by_kind(c)
    bad = []
    for k in A:
        S = C.relrms(Cc[k], A[k])
        err = C.relrms(G[k], A[k])
        if not (S <= S_CEILING_GRAD and err <= 2 * S):
            bad.append((k, err, S))
    return bad, cosine(got, a)


def cosine(x, y):
    X, Y = groups(x), groups(y)
    u, v = torch.cat([X[k] for k in sorted(X)]), torch.cat([Y[k] for k in sorted(Y)])
    return float(u @ v / (u.norm() * v.norm()))
