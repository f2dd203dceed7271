"""WaveGrad test cases without a device: a float64 restatement of the network (written from wavegrad_v190.py) and of the reverse loop
(from examples/wavegrad/reverse.py), the two geometries the GPU tests run, the parameter table and random weights.

`bf16_operands=True` rounds to bf16 exactly where the device does: both operands of every product that runs on MFMA (every
convolution but DBlock[0] and last_conv).  The init convolution, last_conv and the diffusion update stay unrounded."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


class H(dict):
    """A nested dict with attribute access: what the reference's yaml object looks like."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k)
        return H(v) if isinstance(v, dict) else v


SMALL = H(n_mels=64, hop_samples=12, sample_rate=22050, n_fft=2048,
          noise_schedule_start=1e-4, noise_schedule_end=0.05, noise_schedule_S=60,
          dblock=dict(init_conv_channels=32, init_conv_kernels=5, hidden_size=[64, 128], factor=[2, 3], kernel_size=[3, 3, 3],
                      dilations=[1, 2, 4]),
          film=dict(output_size=[64, 128, 128], kernel_size=[3, 3, 3]),
          ublock=dict(hidden_size=[128, 128, 64], factor=[2, 3, 2], dilation=[[1, 2, 1, 2], [1, 2, 4, 8], [1, 2, 4, 8]], kernel_size=3),
          first_conv=dict(hidden_size=128, kernel_size=3), last_conv=dict(kernel_size=3))
SMALL_SHAPE = (2, 20)  # B, frames: T = 240

YAML = H(n_mels=128, hop_samples=300, sample_rate=22050, n_fft=2048,
         noise_schedule_start=0.000001, noise_schedule_end=0.01, noise_schedule_S=1000,
         dblock=dict(init_conv_channels=32, init_conv_kernels=5, hidden_size=[128, 128, 256, 512], factor=[2, 2, 3, 5],
                     kernel_size=[3, 3, 3], dilations=[1, 2, 4]),
         film=dict(output_size=[128, 128, 256, 512, 512], kernel_size=[3, 3, 3, 3, 3]),
         ublock=dict(hidden_size=[512, 512, 256, 128, 128], factor=[5, 5, 3, 2, 2],
                     dilation=[[1, 2, 1, 2], [1, 2, 1, 2], [1, 2, 4, 8], [1, 2, 4, 8], [1, 2, 4, 8]], kernel_size=3),
         first_conv=dict(hidden_size=768, kernel_size=3), last_conv=dict(kernel_size=3))
YAML_SHAPE = (1, 8)  # T = 2400: 8 rows at the coarsest level, the same as the halo

YAML_TEXT = """
sample_rate: 22050
hop_samples: 12
n_fft: 2048
n_mels: 64
noise_schedule_start: 0.0001
noise_schedule_end: 0.05
noise_schedule_S: 60
dblock:
    init_conv_channels: 32
    init_conv_kernels: 5
    hidden_size: [64, 128]
    factor: [2, 3]
    kernel_size: [3, 3, 3]
    dilations: [1, 2, 4]
film:
    output_size: [64, 128, 128]
    kernel_size: [3, 3, 3]
ublock:
    hidden_size: [128, 128, 64]
    factor: [2, 3, 2]
    dilation: [
        [1, 2, 1, 2],
        [1, 2, 4, 8],
        [1, 2, 4, 8]]
    kernel_size: 3
first_conv:
    hidden_size: 128
    kernel_size: 3
last_conv:
    kernel_size: 3
"""


def param_shapes(hps):
    """{state_dict name: shape} as the reference's cells define them (Conv1d weights (out, in, k))."""
    db, fl, ub = hps["dblock"], hps["film"], hps["ublock"]
    out = {}

    def conv(name, cin, cout, k):
        out[name + ".weight"], out[name + ".bias"] = (cout, cin, k), (cout,)

    c0 = db["init_conv_channels"]
    conv("DBlock.0", 1, c0, db["init_conv_kernels"])
    cin = c0
    for n, (hid, f) in enumerate(zip(db["hidden_size"], db["factor"]), 1):
        conv("DBlock.%d.residual_dense" % n, cin, hid, 1)
        conv("DBlock.%d.conv.1" % n, cin, hid, db["kernel_size"][0])
        conv("DBlock.%d.conv.3" % n, hid, hid, db["kernel_size"][1])
        conv("DBlock.%d.conv.5" % n, hid, hid, db["kernel_size"][2])
        conv("DBlock.%d.downscale1" % n, hid, hid, f)
        conv("DBlock.%d.downscale2" % n, cin, cin, f)
        cin = hid
    cin = c0
    for n, (o, k) in enumerate(zip(fl["output_size"], fl["kernel_size"])):
        conv("FiLM.%d.input_conv" % n, cin, cin, k)
        conv("FiLM.%d.output_conv" % n, cin, 2 * o, k)
        cin = o
    cin = hps["first_conv"]["hidden_size"]
    for n, hid in enumerate(ub["hidden_size"]):
        conv("UBlock.%d.block1" % n, cin, hid, 1)
        conv("UBlock.%d.block2_a" % n, cin, hid, ub["kernel_size"])
        for leaf in ("block2_b", "block3_a", "block3_b"):
            conv("UBlock.%d.%s" % (n, leaf), hid, hid, ub["kernel_size"])
        cin = hid
    conv("first_conv", hps["n_mels"], hps["first_conv"]["hidden_size"], hps["first_conv"]["kernel_size"])
    conv("last_conv", ub["hidden_size"][-1], 1, hps["first_conv"]["kernel_size"])
    return out


def make_state(hps, seed):
    """Random float32 weights drawn as the reference initialises them - orthogonal for the Conv1dOrthogonal cells, Xavier-uniform for
    the FiLM and downscale convolutions - plus 0.05 N(0, 1) biases (the reference's are zero; a zero bias would test nothing).  With
    N(0, 1 / fan_in) weights everywhere the network is expansive in the audio and the reverse loop runs away (pred rms 134 after six
    steps); with these it keeps the audio near unit scale, as a vocoder's loop does."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in param_shapes(hps).items():
        if name.endswith(".weight"):
            w = torch.empty(shape)
            if "downscale" in name or name.startswith("FiLM."):
                torch.nn.init.xavier_uniform_(w, generator=g)
            else:
                torch.nn.init.orthogonal_(w, generator=g)
            state[name] = w
        else:
            state[name] = 0.05 * torch.randn(shape, generator=g)
    return state


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def encoding(dim, noise_level):
    """PositionalEncoding.construct (wavegrad_v190.py:84-91) for noise_level (B,) -> (B, dim) float64."""
    count = dim // 2
    step = torch.arange(count, dtype=F64) / count
    e = noise_level.to(F64).unsqueeze(1) * torch.exp(-math.log(1e4) * step.unsqueeze(0))
    return torch.cat([torch.sin(e), torch.cos(e)], -1)


def repeat(x, f):
    """Tensor.repeat(f, 2) of MindSpore = np.repeat along axis 2: [a, b] -> [a, a, b, b]."""
    return torch.repeat_interleave(x, f, dim=2)


def leaky(x):
    return torch.where(x >= 0, x, 0.2 * x)


def film_split(o):
    """ops.split(o, 1, output_num=2): shift is the FIRST half of the channels, scale the second (wavegrad_v190.py:122)."""
    half = o.shape[1] // 2
    return o[:, :half], o[:, half:]


def network(state, hps, audio, noise_level, spectrogram, bf16_operands=False):
    """WaveGrad.forward (wavegrad_v190.py:227-238) in float64, (B, C, T) layout.  audio (B, T), noise_level (B,) or (1,),
    spectrogram (B, n_mels, frames) -> (B, T)."""
    S = {k: v.to(F64) for k, v in state.items()}
    q = bf16 if bf16_operands else (lambda v: v)
    db, ub = hps["dblock"], hps["ublock"]

    def conv(x, name, dilation=1, stride=1, same=True, mfma=True):
        w, b = S[name + ".weight"], S[name + ".bias"]
        pad = (w.shape[-1] // 2) * dilation if same else 0
        if mfma:
            x, w = q(x), q(w)
        return F.conv1d(x, w, b, stride=stride, padding=pad, dilation=dilation)

    level = noise_level.to(F64).reshape(-1)
    x = conv(audio.to(F64).unsqueeze(1), "DBlock.0", mfma=False)
    films = []
    n_levels = len(hps["film"]["output_size"])
    for n in range(n_levels):
        if n > 0:
            f = db["factor"][n - 1]
            residual = conv(x, "DBlock.%d.residual_dense" % n)
            residual = conv(residual, "DBlock.%d.downscale1" % n, stride=f, same=False)
            y = conv(x, "DBlock.%d.downscale2" % n, stride=f, same=False)
            for leaf, d in zip((1, 3, 5), db["dilations"]):
                y = conv(leaky(y), "DBlock.%d.conv.%d" % (n, leaf), dilation=d)
            x = y + residual
        h = leaky(conv(x, "FiLM.%d.input_conv" % n))
        h = h + encoding(h.shape[1], level).unsqueeze(2)
        films.append(film_split(conv(h, "FiLM.%d.output_conv" % n)))
    x = conv(spectrogram.to(F64), "first_conv")
    r2 = math.sqrt(2.0)
    for n, (shift, scale) in enumerate(films[::-1]):
        f, dil = ub["factor"][n], ub["dilation"][n]
        name = "UBlock.%d." % n
        block1 = repeat(conv(x, name + "block1"), f) / f
        block2 = conv(repeat(leaky(x), f) / f, name + "block2_a", dilation=dil[0])
        block2 = conv(leaky((scale * block2 + shift) / r2), name + "block2_b", dilation=dil[1])
        x = (block1 + block2) / r2
        block3 = conv(leaky((scale * x + shift) / r2), name + "block3_a", dilation=dil[2])
        block3 = conv(leaky((scale * block3 + shift) / r2), name + "block3_b", dilation=dil[3])
        x = (x + block3) / r2
    return conv(x, "last_conv", mfma=False).squeeze(1)


def schedule(beta):
    """reverse.py:101-122 in float64 with alpha_cum cast to float32 as the script does (:103).
    -> (noise_level (S,) float32, c1, c2, sigma (S,) float64; sigma[0] is never used and 0 here)."""
    beta = np.asarray(beta, np.float64)
    alpha = 1 - beta
    alpha_cum = np.cumprod(alpha).astype(np.float32)
    S = len(alpha)
    c1 = np.array([1 / alpha[n] ** 0.5 for n in range(S)])
    c2 = np.array([(1 - alpha[n]) / (1 - float(alpha_cum[n])) ** 0.5 for n in range(S)])
    sigma = np.array([0.0] + [((1.0 - float(alpha_cum[n - 1])) / (1.0 - float(alpha_cum[n])) * beta[n]) ** 0.5 for n in range(1, S)])
    return alpha_cum ** 0.5, c1, c2, sigma


def reverse_loop(net, shape, beta, rng=np.random):
    """The loop of reverse.py:105-123 in float64 with the script's np.random call order: first the initial audio, one
    normal(0, 1, [B, T]) cast to float32, then one float64 normal(0, 1, [B, T]) per step with n > 0 (cast to float32 here too: the
    draws the device is fed).  net(audio (B, T) float64 tensor, n) -> pred.  -> (audio float64 ndarray, {m + 1: audio})."""
    level, c1, c2, sigma = schedule(beta)
    S = len(c1)
    audio = rng.normal(0, 1, list(shape)).astype(np.float32).astype(np.float64)
    saved = {}
    for m in range(S):
        n = S - 1 - m
        pred = net(torch.from_numpy(audio), n).numpy()
        audio = c1[n] * (audio - c2[n] * pred)
        if n > 0:
            noise = rng.normal(0, 1, audio.shape).astype(np.float32).astype(np.float64)
            audio = audio + sigma[n] * noise
        if (m + 1) > (S - 50) and (m + 1) % 5 == 0:
            saved[m + 1] = audio.copy()
    return audio, saved


def relrms(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt())


def inputs(hps, shape, seed):
    """audio (B, T) float32, spectrogram (B, n_mels, frames) float32 in [0, 1] like a normalised mel."""
    B, frames = shape
    g = torch.Generator().manual_seed(seed)
    audio = torch.randn((B, hps["hop_samples"] * frames), generator=g)
    spec = torch.rand((B, hps["n_mels"], frames), generator=g)
    return audio, spec
