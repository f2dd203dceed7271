"""The float64 CPU restatement of Conv-TasNet (mindaudio/models/conv_tasnet.py) that test_conv_tasnet_cpu.py / test_conv_tasnet_gpu.py
measure against, written with torch.nn.functional.conv1d on (M, channels, K) tensors - the reference's own layout, not the device's.

forward(state, cfg, mixture, overlap, bf16_operands):
  form (a), bf16_operands=False: exact float64.
  form (b), bf16_operands=True:  the same, but the operands of the four kinds of 1 x 1 convolution - the activations into
            bottleneck_conv1x1, conv1x1, pointwise_conv and mask_conv1x1, and their weights - are rounded to bf16 (through float32,
            as the device produces them).  Nothing else is rounded: (b) differs from (a) only at the points where the device rounds.
S = relrms((b), (a)) is the yardstick of the model tests: the device rounds where (b) rounds, but its bf16 flips are independent of
(b)'s, so two equal independent errors add to sqrt(2) S; the tests allow 2 S, the rest covering float32 accumulation order.

Also here: the reference's 0 / 1 "overlap-add" matrix built as conv_tasnet.py:113-119 builds it, the two-pass float64 SI-SNR of
separation_loss.py:188-216, a brute-force permutation search, and the seeded weights and inputs of the cases.
No figure here is measured on the code under test."""
import itertools
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = os.path.join(HERE, "golden", "separation_sisnr.npz")

EPS = 1e-8
SMALL = dict(N=64, L=20, B=64, H=128, P=3, X=8, R=2, C=2)     # M = 3, T = 3010: K = 300 exceeds the largest dilation (128)
YAML = dict(N=512, L=20, B=256, H=512, P=3, X=8, R=4, C=2)    # examples/conv_tasnet/conv_tasnet.yaml; M = 1, T = 4010
S_CEILING = 3e-2  # a changed restatement cannot widen its own tolerance past this


def relrms(x, ref):
    x, ref = torch.as_tensor(x).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((x - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def param_shapes(N, L, B, H, P, X, R, C):
    """{state-dict name: shape} of mindaudio_amd.models.ConvTasNet, in the reference's cell names."""
    out = {"encoder.conv1d_U.weight": (N, 1, L), "separator.bottleneck_conv1x1.weight": (B, N, 1)}
    for r in range(R):
        for x in range(X):
            p = "separator.temporal_conv_net.%d.%d." % (r, x)
            out[p + "conv1x1.weight"] = (H, B, 1)
            out[p + "prelu.weight"] = (1,)
            out[p + "dsconv.depthwise_conv.weight"] = (H, 1, P)
            out[p + "dsconv.prelu.weight"] = (1,)
            out[p + "dsconv.pointwise_conv.weight"] = (B, H, 1)
    out["separator.mask_conv1x1.weight"] = (C * N, B, 1)
    out["decoder.basis_signals.weight"] = (L, N)
    return out


def make_state(cfg, seed):
    """He-uniform float32 weights (bound sqrt(6 / fan_in)); PReLU weights drawn around the default 0.25 so that each one matters."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in param_shapes(**cfg).items():
        if len(shape) == 1:
            state[name] = (0.25 + 0.1 * (torch.rand(shape, generator=g) - 0.5)).float()
        else:
            fan_in = int(np.prod(shape[1:]))
            bound = (6.0 / fan_in) ** 0.5
            state[name] = ((torch.rand(shape, generator=g) * 2 - 1) * bound).float()
    return state


def make_mixture(M, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn((M, T), generator=g)).float()


def gln(y):
    """GlobalLayerNorm (conv_tasnet.py:450-463) on (M, channels, K): gamma = 1, beta = 0."""
    mean = y.mean(dim=(1, 2), keepdim=True)
    var = (y - mean).pow(2).mean(dim=(1, 2), keepdim=True)
    return (y - mean) / torch.sqrt(var + EPS)


def paired_matrix(K):
    """conv_tasnet.py:113-119 for K frames: (2K, K) with ones at [2i, i] and [2i + 1, i]."""
    alpha = np.zeros((2 * K, K), np.float64)
    for i in range(K):
        alpha[2 * i, i] = 1
        alpha[2 * i + 1, i] = 1
    return torch.from_numpy(alpha)


def overlap_paired_reference(frames):
    """Decoder.overlap_and_add of the reference (conv_tasnet.py:148-190) on frames (M, C, K, L), with its matrix sized for K: the
    frames viewed as subframes of L / 2, transposed, multiplied by the 0 / 1 matrix, transposed back and flattened."""
    M, C, K, L = frames.shape
    sub = frames.reshape(M, C, -1, L // 2)            # (M, C, 2K, L/2)
    res = torch.matmul(sub.transpose(2, 3), paired_matrix(K).to(frames.dtype))  # (M, C, L/2, K)
    return res.transpose(2, 3).reshape(M, C, -1)       # (M, C, K * L/2)


def overlap_paired(frames):
    """out[k L/2 + j] = frame_k[j] + frame_k[j + L/2], then L / 2 zeros (the model's pad; 10 at the reference's L = 20)."""
    M, C, K, L = frames.shape
    h = L // 2
    body = (frames[..., :h] + frames[..., h:]).reshape(M, C, K * h)
    return torch.cat([body, body.new_zeros(M, C, h)], dim=2)


def overlap_true(frames):
    """The real overlap-add: out[k L/2 + j] += frame_k[j], length (K + 1) L / 2."""
    M, C, K, L = frames.shape
    h = L // 2
    out = frames.new_zeros(M, C, (K + 1) * h)
    for k in range(K):
        out[:, :, k * h:k * h + L] += frames[:, :, k]
    return out


def forward(state, cfg, mixture, overlap="paired", bf16_operands=False):
    N, L, B, H, P, X, R, C = (cfg[k] for k in "NLBHPXRC")
    rnd = bf16_round if bf16_operands else (lambda t: t)
    w = {k: v.double() for k, v in state.items()}
    x = mixture.double()
    M = x.shape[0]
    mixture_w = F.relu(F.conv1d(x[:, None, :], w["encoder.conv1d_U.weight"], stride=L // 2))  # (M, N, K)
    K = mixture_w.shape[2]
    y = F.conv1d(rnd(gln(mixture_w)), rnd(w["separator.bottleneck_conv1x1.weight"]))
    for r in range(R):
        for xi in range(X):
            p = "separator.temporal_conv_net.%d.%d." % (r, xi)
            d = 2 ** xi
            t = F.conv1d(rnd(y), rnd(w[p + "conv1x1.weight"]))
            t = gln(F.prelu(t, w[p + "prelu.weight"]))
            t = F.conv1d(t, w[p + "dsconv.depthwise_conv.weight"], padding=(P - 1) * d // 2, dilation=d, groups=H)
            t = gln(F.prelu(t, w[p + "dsconv.prelu.weight"]))
            y = y + F.conv1d(rnd(t), rnd(w[p + "dsconv.pointwise_conv.weight"]))
    score = F.conv1d(rnd(y), rnd(w["separator.mask_conv1x1.weight"])).view(M, C, N, K)
    source_w = (mixture_w[:, None] * F.relu(score)).transpose(2, 3)  # (M, C, K, N)
    frames = source_w @ w["decoder.basis_signals.weight"].t()         # (M, C, K, L)
    return overlap_paired(frames) if overlap == "paired" else overlap_true(frames)


def si_snr_pairwise(source, estimate, lengths):
    """separation_loss.py:188-216 in float64 NumPy, masked by the lengths: [b, i_est, j_target]."""
    source, estimate = np.asarray(source, np.float64), np.asarray(estimate, np.float64)
    Bn, C, _ = source.shape
    out = np.zeros((Bn, C, C))
    for b in range(Bn):
        n = int(lengths[b])
        for i in range(C):
            for j in range(C):
                e, t = estimate[b, i, :n], source[b, j, :n]
                e, t = e - e.sum() / n, t - t.sum() / n
                proj = np.sum(e * t) * t / (np.sum(t ** 2) + EPS)
                noise = e - proj
                out[b, i, j] = 10 * np.log(np.sum(proj ** 2) / (np.sum(noise ** 2) + EPS) + EPS) / np.log(10.0)
    return out


def write_wav(path, samples, rate=8000):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples, "<i2").tobytes())


def make_dataset(root, lengths, seed=0):
    """mix_clean.json / s1.json / s2.json over seeded 16-bit 8 kHz wavs (s1, s2 and their sum), listed in the order given;
    returns {length: (s1, s2) as the int16 arrays written}."""
    import json

    rng = np.random.RandomState(seed)
    lists = {"mix_clean": [], "s1": [], "s2": []}
    written = {}
    for idx, n in enumerate(lengths):
        s1 = (rng.randn(n) * 3000).astype(np.int16)
        s2 = (rng.randn(n) * 3000).astype(np.int16)
        arrays = {"mix_clean": (s1.astype(np.int32) + s2).astype(np.int16), "s1": s1, "s2": s2}
        for kind, arr in arrays.items():
            d = os.path.join(root, kind)
            os.makedirs(d, exist_ok=True)
            p = os.path.join(d, "utt%d.wav" % idx)
            write_wav(p, arr)
            lists[kind].append([p, n])
        written[n] = (s1, s2)
    for kind, items in lists.items():
        with open(os.path.join(root, kind + ".json"), "w") as f:
            json.dump(items, f)
    return written


def best_permutation(pair):
    """Brute force over itertools.permutations(range(C)), the first wins ties: (perm, sum / C) of one utterance's (C, C) table."""
    C = pair.shape[0]
    best, best_perm = None, None
    for perm in itertools.permutations(range(C)):
        s = sum(pair[perm[j], j] for j in range(C))
        if best is None or s > best:
            best, best_perm = s, perm
    return best_perm, best / C
