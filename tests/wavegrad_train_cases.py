"""The CPU reference side of WaveGrad training (test_wavegrad_train_cpu.py / test_wavegrad_train_gpu.py): the network of
wavegrad_cases.network restated over a dtype and a pluggable convolution, the L1 loss, gradients by torch.autograd in three forms,
ops.clip_by_global_norm and nn.Adam as MyTrainOneStepCell chains them, the learning-rate schedule, the cases, the guard and the
comparators.

  form "a": exact float64.
  form "b": float32 throughout - the same code on .float() tensors.
  form "c": float64 with the operands of every MFMA product rounded to bf16 in the forward AND in the backward (dY and the saved
            operands, where the device rounds: dX = bf16(dY) * bf16(W), dW = bf16(dY) * bf16(X), db = sum bf16(dY)).

Nothing here imports the code under test, and no figure here is measured on it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import wavegrad_cases as W
from conv_tasnet_train_cases import COS_MIN, FLIP_GUARD, MARGIN, S_CEILING_GRAD  # noqa: F401  (the project's constants)

# nn.Adam's defaults as the float32 parameters they are, and 1 - beta as the float32 subtraction gives it (1 - 0.999f is 4.7e-5 above
# 0.001: a float64 restatement with the decimal constants would differ from any float32 Adam by that much in the second moment)
BETA1, BETA2, ADAM_EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
ONE_MINUS_BETA1, ONE_MINUS_BETA2 = float(np.float32(1.0) - np.float32(0.9)), float(np.float32(1.0) - np.float32(0.999))

# Channel counts that are multiples of 8 but not of 64 (C = 8 and 16 under Cpad = 64), every repetition factor of the yaml (2, 3, 5)
TINY = W.H(n_mels=8, hop_samples=30, sample_rate=22050, n_fft=2048,
           noise_schedule_start=1e-4, noise_schedule_end=0.05, noise_schedule_S=60,
           dblock=dict(init_conv_channels=8, init_conv_kernels=3, hidden_size=[8, 16], factor=[2, 3], kernel_size=[3, 3, 3],
                       dilations=[1, 2, 4]),
           film=dict(output_size=[8, 16, 16], kernel_size=[3, 3, 3]),
           ublock=dict(hidden_size=[16, 16, 8], factor=[5, 3, 2], dilation=[[1, 2, 1, 2], [1, 2, 4, 8], [1, 2, 4, 8]], kernel_size=3),
           first_conv=dict(hidden_size=16, kernel_size=3), last_conv=dict(kernel_size=3))

#        name       hps      (B, frames)
CASES = {"tiny_b2": (TINY, (2, 3)),
         "tiny_b3": (TINY, (3, 2)),
         "tiny_1f": (TINY, (2, 1)),       # one frame: 5 rows at the coarsest level, below every dilation but 1, 2, 4
         "small": (W.SMALL, W.SMALL_SHAPE),
         "yaml": (W.YAML, W.YAML_SHAPE)}  # coarsest level 8 rows = the halo, factor 5, 768 channels
F32_CASES = ("tiny_b2", "tiny_b3", "tiny_1f", "small")
BF16_CASES = ("small", "yaml")


def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------
def plain_conv(x, w, b, stride, pad, dilation):
    return F.conv1d(x, w, b, stride=stride, padding=pad, dilation=dilation)


def rounded_conv(x, w, b, stride, pad, dilation):
    """bf16 operands in the forward only (what wavegrad_cases.network does with bf16_operands=True)."""
    return F.conv1d(bf16_round(x), bf16_round(w), b, stride=stride, padding=pad, dilation=dilation)


class _Bf16Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dilation):
        xr, wr = bf16_round(x), bf16_round(w)
        ctx.save_for_backward(xr, wr)
        ctx.geom = (stride, pad, dilation)
        return F.conv1d(xr, wr, b, stride=stride, padding=pad, dilation=dilation)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        stride, pad, dilation = ctx.geom
        dyr = bf16_round(dy)
        dx = torch.nn.grad.conv1d_input(xr.shape, wr, dyr, stride=stride, padding=pad, dilation=dilation)
        dw = torch.nn.grad.conv1d_weight(xr, wr.shape, dyr, stride=stride, padding=pad, dilation=dilation)
        return dx, dw, dyr.sum(dim=(0, 2)), None, None, None


def bf16_conv(x, w, b, stride, pad, dilation):
    return _Bf16Conv.apply(x, w, b, stride, pad, dilation)


# ---- planted defects (the comparators must reject each) ----------------------------------------------------------------------------------
class _DroppedTapConv(torch.autograd.Function):
    """A convolution whose weight gradient lacks its first tap."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dilation):
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, pad, dilation)
        return F.conv1d(x, w, b, stride=stride, padding=pad, dilation=dilation)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, dilation = ctx.geom
        dx = torch.nn.grad.conv1d_input(x.shape, w, dy, stride=stride, padding=pad, dilation=dilation)
        dw = torch.nn.grad.conv1d_weight(x, w.shape, dy, stride=stride, padding=pad, dilation=dilation).clone()
        if w.shape[2] > 1:
            dw[:, :, 0] = 0
        return dx, dw, dy.sum(dim=(0, 2)), None, None, None


class _RepeatNoDivide(torch.autograd.Function):
    """repeat(x, f) / f whose backward sums the f rows without the 1 / f."""

    @staticmethod
    def forward(ctx, x, f):
        ctx.f = f
        return W.repeat(x, f) / f

    @staticmethod
    def backward(ctx, dy):
        return dy.reshape(dy.shape[0], dy.shape[1], -1, ctx.f).sum(3), None


class _FilmSwapped(torch.autograd.Function):
    """scale * x + shift whose backward hands the shift's gradient to the scale and the other way round."""

    @staticmethod
    def forward(ctx, scale, x, shift):
        ctx.save_for_backward(scale, x)
        return scale * x + shift

    @staticmethod
    def backward(ctx, dy):
        scale, x = ctx.saved_tensors
        return dy, dy * scale, dy * x


class _LeakyNoMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return torch.where(x >= 0, x, 0.2 * x)

    @staticmethod
    def backward(ctx, dy):
        return dy


class _L1SignOfZeroIsOne(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d):
        ctx.save_for_backward(d)
        return d.abs().mean()

    @staticmethod
    def backward(ctx, dy):
        (d,) = ctx.saved_tensors
        return dy * torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d)) / d.numel()


DEFECTS = ("tap", "rep", "film", "mask")


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def network(w, hps, audio, noise_level, spectrogram, conv=plain_conv, defect=None, sites=None):
    """wavegrad_cases.network on the tensors of `w` as they are (their dtype, their autograd state), (B, C, T) layout.  `conv` runs
    every convolution that is an MFMA product on the device (all but DBlock.0 and last_conv).  `sites`: a list that receives the input
    of every LeakyReLU."""
    dtype = audio.dtype
    db, ub = hps["dblock"], hps["ublock"]
    mfma_conv = _DroppedTapConv.apply if defect == "tap" else conv

    def cv(x, name, dilation=1, stride=1, same=True, mfma=True):
        wt, b = w[name + ".weight"], w[name + ".bias"]
        pad = (wt.shape[-1] // 2) * dilation if same else 0
        return (mfma_conv if mfma else plain_conv)(x, wt, b, stride, pad, dilation)

    def leaky(x):
        if sites is not None:
            sites.append(x.detach())
        return _LeakyNoMask.apply(x) if defect == "mask" else torch.where(x >= 0, x, 0.2 * x)

    def rep(x, f):
        return _RepeatNoDivide.apply(x, f) if defect == "rep" else W.repeat(x, f) / f

    def film(scale, x, shift):
        return _FilmSwapped.apply(scale, x, shift) if defect == "film" else scale * x + shift

    level = noise_level.to(torch.float64).reshape(-1)
    x = cv(audio.unsqueeze(1), "DBlock.0", mfma=False)
    films = []
    n_levels = len(hps["film"]["output_size"])
    for n in range(n_levels):
        if n > 0:
            f = db["factor"][n - 1]
            residual = cv(x, "DBlock.%d.residual_dense" % n)
            residual = cv(residual, "DBlock.%d.downscale1" % n, stride=f, same=False)
            y = cv(x, "DBlock.%d.downscale2" % n, stride=f, same=False)
            for leaf, d in zip((1, 3, 5), db["dilations"]):
                y = cv(leaky(y), "DBlock.%d.conv.%d" % (n, leaf), dilation=d)
            x = y + residual
        h = leaky(cv(x, "FiLM.%d.input_conv" % n))
        h = h + W.encoding(h.shape[1], level).unsqueeze(2).to(dtype)
        films.append(W.film_split(cv(h, "FiLM.%d.output_conv" % n)))
    x = cv(spectrogram, "first_conv")
    r2 = math.sqrt(2.0)
    for n, (shift, scale) in enumerate(films[::-1]):
        f, dil = ub["factor"][n], ub["dilation"][n]
        name = "UBlock.%d." % n
        block1 = rep(cv(x, name + "block1"), f)
        block2 = cv(rep(leaky(x), f), name + "block2_a", dilation=dil[0])
        block2 = cv(leaky(film(scale, block2, shift) / r2), name + "block2_b", dilation=dil[1])
        x = (block1 + block2) / r2
        block3 = cv(leaky(film(scale, x, shift) / r2), name + "block3_a", dilation=dil[2])
        block3 = cv(leaky(film(scale, block3, shift) / r2), name + "block3_b", dilation=dil[3])
        x = (x + block3) / r2
    return cv(x, "last_conv", mfma=False).squeeze(1)


def l1_loss(pred, noise, defect=None):
    """nn.L1Loss() of train.py:32: mean |pred - noise|; torch's sign(0) is 0, as the device's."""
    d = pred - noise
    return _L1SignOfZeroIsOne.apply(d) if defect == "sign0" else d.abs().mean()


_FORMS = {"a": (torch.float64, plain_conv), "b": (torch.float32, plain_conv), "c": (torch.float64, bf16_conv)}


def grads(state, hps, batch, form="a", defect=None, loss_scale=1.0, sites=None):
    """(loss, {name: d(loss_scale * loss) / d parameter}, {"pred": the same for the network's output, "value": pred}) by torch.autograd.
    batch = (noisy_audio, noise_level, noise, spectrogram)."""
    dtype, conv = _FORMS[form]
    w = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    audio, level, noise, spec = batch
    pred = network(w, hps, audio.to(dtype), level, spec.to(dtype), conv, defect, sites)
    pred.retain_grad()
    d = pred - noise.to(dtype)
    if sites is not None:
        sites.append(d.detach())
    value = l1_loss(pred, noise.to(dtype), defect)
    (value * loss_scale).backward()
    return float(value.detach()), {k: v.grad.detach() for k, v in w.items()}, {"pred": pred.grad.detach(), "value": pred.detach()}


# ---- the optimizer ------------------------------------------------------------------------------------------------------------------------
def clip_adam_step(params, grads_, m1, m2, t, lr, loss_scale, clip, defect=None):
    """MyTrainOneStepCell (train.py:44-60) on dicts of tensors, in place: grads / loss_scale, ops.clip_by_global_norm(grads, clip) =
    grads * clip / max(norm, clip), nn.Adam with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), t the 1-based step.  -> the norm."""
    names = sorted(params)
    if defect == "clip":  # clipping before unscaling
        norm = math.sqrt(sum(float(grads_[k].double().pow(2).sum()) for k in names))
        factor = clip / max(norm, clip) / loss_scale
    else:
        norm = math.sqrt(sum(float((grads_[k].double() / loss_scale).pow(2).sum()) for k in names))
        factor = clip / max(norm, clip) / loss_scale
    lr_t = lr * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    for k in names:
        g = grads_[k] * factor
        m1[k].mul_(BETA1).add_(ONE_MINUS_BETA1 * g)
        m2[k].mul_(BETA2).add_(ONE_MINUS_BETA2 * g * g)
        params[k].sub_(lr_t * m1[k] / (m2[k].sqrt() + ADAM_EPS))
    return norm


def trajectory(state, hps, batch, form, steps, lr, loss_scale=1.0, clip=1.0):
    """The losses BEFORE each of `steps` steps on one batch, and the loss after the last, in the form's arithmetic."""
    dtype = _FORMS[form][0]
    params = {k: v.detach().to(dtype).clone() for k, v in state.items()}
    m1, m2 = {k: torch.zeros_like(v) for k, v in params.items()}, {k: torch.zeros_like(v) for k, v in params.items()}
    out = []
    for i in range(steps):
        value, g, _ = grads(params, hps, batch, form, loss_scale=loss_scale)
        out.append(value)
        clip_adam_step(params, g, m1, m2, i + 1, lr, loss_scale, clip)
    out.append(grads(params, hps, batch, form)[0])
    return out


def exponential_decay_lr(lr, decay_rate, total_step, step_per_epoch, decay_epoch, is_stair=True):
    """nn.exponential_decay_lr in closed form: lr * decay_rate ** (epoch / decay_epoch), floored when is_stair, epoch = i // per_epoch."""
    out = []
    for i in range(total_step):
        e = (i // step_per_epoch) / decay_epoch
        out.append(lr * decay_rate ** (math.floor(e) if is_stair else e))
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def flip_margin(state, hps, batch):
    """How far every LeakyReLU input and every pred - noise stay from zero, in units of FLIP_GUARD x the float32 error there (the rule
    of conv_tasnet_train_cases.flip_margin): the smallest |v_a| / (FLIP_GUARD max(|v_b - v_a|, rms(v_b - v_a))) over every element,
    v_a from form (a), v_b from form (b).  No element is excluded."""
    sa, sb = [], []
    grads(state, hps, batch, "a", sites=sa)
    grads(state, hps, batch, "b", sites=sb)
    worst = float("inf")
    for a, b in zip(sa, sb):
        a, b = a.double(), b.double()
        err = (b - a).abs()
        guard = FLIP_GUARD * torch.maximum(err, err.pow(2).mean().sqrt())
        worst = min(worst, float((a.abs() / guard).min()))
    return worst


def make_batch(hps, shape, seed):
    audio, spec = W.inputs(hps, shape, seed)
    g = torch.Generator().manual_seed(seed + 7)
    noise = torch.randn(audio.shape, generator=g)
    level = 0.2 + 0.7 * torch.rand((shape[0],), generator=g)
    return audio, level, noise, spec


SEEDS = {"tiny_b2": 1, "tiny_b3": 2, "tiny_1f": 3, "small": 4, "yaml": 5}  # the first of seed, seed + 1000, ... that satisfies the guard
_made, _ref = {}, {}


def case(name):
    """dict(hps, shape, state, batch): built once and shared; nobody changes it."""
    if name not in _made:
        hps, shape = CASES[name]
        seed = SEEDS[name]
        _made[name] = dict(hps=hps, shape=shape, state=W.make_state(hps, 20 + seed), batch=make_batch(hps, shape, seed))
    return _made[name]


def search_seed(name, tries=64):
    """The first seed of SEEDS[name] % 1000 + 1000 k whose flip_margin is at least 1 (run on the CPU when a case is added)."""
    hps, shape = CASES[name]
    base = SEEDS[name] % 1000
    for k in range(tries):
        seed = base + 1000 * k
        if flip_margin(W.make_state(hps, 20 + seed), hps, make_batch(hps, shape, seed)) >= 1.0:
            return seed
    raise AssertionError("no seed keeps the masks clear of zero")


def reference(name, form, loss_scale=1.0):
    key = (name, form, loss_scale)
    if key not in _ref:
        c = case(name)
        _ref[key] = grads(c["state"], c["hps"], c["batch"], form, loss_scale=loss_scale)
    return _ref[key]


# ---- comparators --------------------------------------------------------------------------------------------------------------------------
def relrms(a, b):
    return W.relrms(a, b)


def flat(g):
    return {k: torch.as_tensor(v).detach().double().cpu().reshape(-1) for k, v in g.items()}


def kind(name):
    """The parameter group of a tensor in bf16 mode: the cell's role over all levels, weight and bias together."""
    for key in ("residual_dense", "downscale", "input_conv", "output_conv", "block1", "block2_a", "block2_b", "block3_a", "block3_b",
                "first_conv", "last_conv", "DBlock.0"):
        if key in name:
            return key
    if ".conv." in name:
        return "dblock_conv"
    raise KeyError(name)


def _grouped(g, key):
    out = {}
    for k, v in sorted(flat(g).items()):
        out.setdefault(key(k), []).append(v)
    return {k: torch.cat(v) for k, v in out.items()}


def by_kind(g):
    return _grouped(g, kind)


def by_cell(g):
    """The parameter group in float32 mode: one cell, its weight and its bias together.  (A bias of one element - last_conv's - has no
    rms of its own: form (b)'s error of a single float32 number lies anywhere between zero and its rounding bound, so a multiple of it
    bounds nothing.  conv_tasnet_train_cases gathers the one-element PReLU slopes for the same reason.)"""
    return _grouped(g, lambda name: name.rsplit(".", 1)[0])


def check_f32(got, a, b):
    """Every cell of `got` within MARGIN x relrms(b, a) of (a); returns the list of failures (name, got, allowed)."""
    G, A, Bf = by_cell(got), by_cell(a), by_cell(b)
    bad = []
    for k in A:
        allowed = MARGIN * relrms(Bf[k], A[k])
        err = relrms(G[k], A[k])
        if not err <= allowed:
            bad.append((k, err, allowed))
    return bad


def check_bf16(got, a, c):
    """Per parameter group relrms(got, a) <= 2 S, S = relrms(c, a) <= S_CEILING_GRAD; -> (failures, {group: (err, S)}, cosine)."""
    G, A, Cc = by_kind(got), by_kind(a), by_kind(c)
    bad, table = [], {}
    for k in A:
        S = relrms(Cc[k], A[k])
        err = relrms(G[k], A[k])
        table[k] = (err, S)
        if not (S <= S_CEILING_GRAD and err <= 2 * S):
            bad.append((k, err, S))
    return bad, table, cosine(got, a)


def cosine(x, y):
    X, Y = flat(x), flat(y)
    u, v = torch.cat([X[k] for k in sorted(X)]), torch.cat([Y[k] for k in sorted(Y)])
    return float(u @ v / (u.norm() * v.norm()))
