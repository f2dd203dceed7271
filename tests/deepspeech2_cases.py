"""The float64 NumPy restatement of DeepSpeech2 (mindaudio/models/deepspeech2.py, examples/deepspeech2/{eval,dataset}.py,
mindaudio/models/decoders/greedydecoder.py) that test_deepspeech2_cpu.py / test_deepspeech2_gpu.py measure against, in the reference's
own layouts: x (B, 1, F, T), conv weights (out, in, kf, kt), LSTM input (T1, B, 32 * F2) with feature c * F2 + f.

Two forms of every stage:
  exact         float64 throughout.
  rounding-only the same float64 arithmetic with values rounded to bf16 (through float32, round to nearest even) at exactly the
                points where the device rounds: conv1's output; conv2's weights and output; in every LSTM layer x, W_ih, W_hh and the h
                that is fed back; the fc input and weight.  Projections, gate sums, c and the layer outputs are never rounded.
S = relrms(rounding-only, exact) is the yardstick; the device tests allow 2 S, the factor covering float32 accumulation order and
float32 sigmoid / tanh, which the rounding-only form lacks.  No figure here is measured on the code under test."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
WAV = os.path.join(HERE, "golden", "BAC009S0002W0122.wav")
BN_EPS = 1e-5
LABELS = ["'", "A", "B", "C", "D", "E", "F", "G", "H", "I", "J", "K", "L", "M", "N", "O", "P", "Q", "R", "S", "T", "U", "V", "W", "X",
          "Y", "Z", " ", "_"]  # deepspeech2.yaml

SMALL = dict(sample_rate=1600, window_size=0.02, H=64, layers=2, B=3, T=45)         # F = 17, LSTM input 160
YAML_GEOMETRY = dict(sample_rate=16000, window_size=0.02, H=1024, layers=2, B=2, T=40)  # F = 161, LSTM input 1312


def relrms(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def n_freq(sample_rate, window_size):
    return int(np.floor(sample_rate * window_size / 2) + 1)


def conv_out(n, k, pad, stride):
    return (n + 2 * pad - k) // stride + 1


def get_seq_lens(seq_len):
    """deepspeech2.py:266-286: pre = 2 * 5 - 1 * (11 - 1) - 1 = -1 for both convolutions, strides 2 and 1, on int32."""
    v = np.asarray(seq_len).astype(np.int32)
    for pre, stride in ((-1, 2), (-1, 1)):
        v = ((v + pre) / stride).astype(np.int32) + 1  # int32 Div: the quotient truncated (the numerator is >= 0 for len >= 1)
    return v


# ---- MaskConv ---------------------------------------------------------------------------------------------------------------------------
def conv2d(x, w, stride, pad):
    """x (B, Cin, F, T), w (Cout, Cin, kf, kt) float64, cross-correlation as nn.Conv2d, zero padding (pf, pt), no bias."""
    B, Cin, F, T = x.shape
    Cout, _, kf, kt = w.shape
    (sf, st), (pf, pt) = stride, pad
    Fo, To = conv_out(F, kf, pf, sf), conv_out(T, kt, pt, st)
    xp = np.zeros((B, Cin, F + 2 * pf, T + 2 * pt))
    xp[:, :, pf:pf + F, pt:pt + T] = x
    out = np.zeros((B, Cout, Fo, To))
    for a in range(kf):
        for b in range(kt):
            sl = xp[:, :, a:a + sf * (Fo - 1) + 1:sf, b:b + st * (To - 1) + 1:st]
            out += np.einsum("oc,bcft->boft", w[:, :, a, b], sl)
    return out


def batchnorm(x, p, prefix):
    g, b, m, v = (np.asarray(p[prefix + k], np.float64)[None, :, None, None] for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    return (x - m) / np.sqrt(v + BN_EPS) * g + b


def mask_conv(p, x, rounding=False, stage1_only=False):
    """(B, 1, F, T) -> (B, 32, F2, T1); nothing is masked."""
    r = bf16_round if rounding else (lambda a: a)
    w1, w2 = np.asarray(p["conv.conv1.weight"], np.float64), np.asarray(p["conv.conv2.weight"], np.float64)
    y = r(np.tanh(batchnorm(conv2d(np.asarray(x, np.float64), w1, (2, 2), (20, 5)), p, "conv.bn1.")))
    if stage1_only:
        return y
    return r(np.tanh(batchnorm(conv2d(y, r(w2), (2, 1), (10, 5)), p, "conv.bn2.")))


def conv1_abs_terms(p, x):
    """sum over the 451 taps of |w x| per output (B, 32, F1, T1): the scale of conv1's float32 accumulation bound."""
    return conv2d(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(p["conv.conv1.weight"], np.float64)), (2, 2), (20, 5))


# ---- LSTM -------------------------------------------------------------------------------------------------------------------------------
def lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse, rounding=False, stats=None):
    """One direction of nn.LSTM on x (T, B, K): gate order i, f, g, o; h0 = c0 = 0; the reverse direction walks t = T - 1 .. 0 and
    writes at index t.  -> (h (T, B, H), c after the last step (B, H))."""
    r = bf16_round if rounding else (lambda a: a)
    x, w_ih, w_hh = r(np.asarray(x, np.float64)), r(np.asarray(w_ih, np.float64)), r(np.asarray(w_hh, np.float64))
    bias = np.asarray(b_ih, np.float64) + np.asarray(b_hh, np.float64)
    T, B, _ = x.shape
    H = w_hh.shape[1]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    out = np.zeros((T, B, H))
    for s in range(T):
        t = T - 1 - s if reverse else s
        gates = x[t] @ w_ih.T + bias + r(h) @ w_hh.T
        if stats is not None:
            stats.append(float(np.abs(gates).min()))
        i, f, g, o = (gates[:, k * H:(k + 1) * H] for k in range(4))
        c = sigmoid(f) * c + sigmoid(i) * np.tanh(g)
        h = sigmoid(o) * np.tanh(c)
        out[t] = h
    return out, c


def lstm_bidir(x, layer, rounding=False, dirs=(0, 1), stats=None):
    """A bidirectional layer with the directions SUMMED (deepspeech2.py:183-186).  layer: {weight_ih, weight_hh, bias_ih, bias_hh} each
    (2, ...) stacked forward / reverse.  -> (out (T, B, H), c_final (2, B, H))."""
    T, B, _ = np.shape(x)
    H = layer["weight_hh"].shape[2]
    out, cs = np.zeros((T, B, H)), np.zeros((2, B, H))
    for d in dirs:
        h, c = lstm_direction(x, layer["weight_ih"][d], layer["weight_hh"][d], layer["bias_ih"][d], layer["bias_hh"][d], d == 1,
                              rounding, stats)
        out += h
        cs[d] = c
    return out, cs


def lstm_layer_params(seed, K, H):
    """uniform(+-1 / sqrt(H)) float32, both directions stacked."""
    g = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(H)
    return {n: g.uniform(-k, k, (2,) + s).astype(np.float32) for n, s in
            (("weight_ih", (4 * H, K)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,)))}


def layer_of(p, k):
    pre = "RNN.lstms.%d." % k
    return {n: np.stack([np.asarray(p[pre + n + "_l0"]), np.asarray(p[pre + n + "_l0_reverse"])]) for n in
            ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}


# ---- routing case: saturated gates ----------------------------------------------------------------------------------------------------------
def routing_case(T, B, H, K=64, seed=0):
    """One layer whose every gate is saturated, so that h and c move in steps of the saturated cell and a swapped gate, a reversed time
    index, a wrong hidden slice or a wrong batch row changes the result by O(1).  gate = a + b + r with
      a  the input part: x[t, b] is one-hot at column (3 t + 5 b + 1) % K and W_ih is 0 or +-128 -> a in {0, +-128};
      b  bias_ih = +-32, bias_hh = 0;
      r  the recurrent part: ONE non-zero W_hh entry per gate row, +-64, at a column that depends on the gate, the unit and the
         direction; |h| = sigmoid(o) |tanh(c)| with |c| >= 1 or c == 0, so r is 0 or 64 |h| in [48.7, 64].
    Every value is exact in bf16 (the fed-back h is not, but its rounding moves a gate by < 0.01) and |a + b + r| >= 16.7 whatever the
    signs, so every sigmoid is within 1 - sigmoid(16.7) = 5.6e-8 of 0 or 1 and tanh(g) within 1e-14 of +-1: the float64 restatement
    and a correct float32 kernel differ by the saturation residues accumulated over T <= 7 steps, below the bound 1e-6.
    The patterns differ per direction, per gate row (hence per hidden slice) and per batch row (through x)."""
    g = np.random.RandomState(1000 + seed + 7 * T + 13 * B + H)
    x = np.zeros((T, B, K), np.float32)
    for t in range(T):
        for b in range(B):
            x[t, b, (3 * t + 5 * b + 1) % K] = 1.0
    w_ih = (g.randint(-1, 2, (2, 4 * H, K)) * 128).astype(np.float32)
    b_ih = (g.choice([-32.0, 32.0], (2, 4 * H))).astype(np.float32)
    w_hh = np.zeros((2, 4 * H, H), np.float32)
    for d in range(2):
        for gate in range(4):
            for j in range(H):
                w_hh[d, gate * H + j, (7 * j + 3 + gate + 5 * d) % H] = g.choice([-64.0, 64.0])
    return x, dict(weight_ih=w_ih, weight_hh=w_hh, bias_ih=b_ih, bias_hh=np.zeros_like(b_ih))


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def param_shapes(sample_rate, window_size, H, layers, n_labels=len(LABELS), **_):
    F = n_freq(sample_rate, window_size)
    F2 = conv_out(conv_out(F, 41, 20, 2), 21, 10, 2)
    out = {"conv.conv1.weight": (32, 1, 41, 11), "conv.conv2.weight": (32, 32, 21, 11)}
    for bn in ("conv.bn1.", "conv.bn2."):
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            out[bn + k] = (32,)
    for k in range(layers):
        K = 32 * F2 if k == 0 else H
        for suffix in ("", "_reverse"):
            pre = "RNN.lstms.%d." % k
            out[pre + "weight_ih_l0" + suffix] = (4 * H, K)
            out[pre + "weight_hh_l0" + suffix] = (4 * H, H)
            out[pre + "bias_ih_l0" + suffix] = (4 * H,)
            out[pre + "bias_hh_l0" + suffix] = (4 * H,)
    out["fc.module.weight"] = (n_labels, H)
    return out


def make_state(cfg, seed):
    """Seeded float32 weights: convolutions normal(0, sqrt(2 / (kf kt out))) as the reference initialises them, BatchNorm statistics
    away from the identity so that each one matters, LSTM uniform(+-1 / sqrt(H)), fc uniform(+-1 / sqrt(H))."""
    g = np.random.RandomState(seed)
    H = cfg["H"]
    state = {}
    for name, shape in param_shapes(**cfg).items():
        leaf = name.rsplit(".", 1)[1]
        if name.startswith("conv.conv"):
            v = g.normal(0.0, np.sqrt(2.0 / (shape[2] * shape[3] * shape[0])), shape)
        elif leaf == "gamma":
            v = g.uniform(0.8, 1.2, shape)
        elif leaf == "moving_variance":
            v = g.uniform(0.5, 1.5, shape)
        elif leaf in ("beta", "moving_mean"):
            v = g.uniform(-0.2, 0.2, shape)
        else:
            v = g.uniform(-1.0, 1.0, shape) / np.sqrt(H)
        state[name] = v.astype(np.float32)
    return state


def make_input(cfg, seed, B=None, T=None, pad_frames=0):
    """A (B, 1, F, T) float32 'normalised spectrogram' (unit normal), its last pad_frames frames zero like the eval padding."""
    B, T = B or cfg["B"], T or cfg["T"]
    F = n_freq(cfg["sample_rate"], cfg["window_size"])
    x = np.random.RandomState(seed).normal(0.0, 1.0, (B, 1, F, T)).astype(np.float32)
    if pad_frames:
        x[..., T - pad_frames:] = 0.0
    return x


def rnn_input(y):
    """(B, 32, F2, T1) -> (T1, B, 32 * F2), feature c * F2 + f (deepspeech2.py:259-261)."""
    B, C, F2, T1 = y.shape
    return y.reshape(B, C * F2, T1).transpose(2, 0, 1)


def forward(p, cfg, x, rounding=False):
    """-> (logits (T1, B, classes), the LSTM stack's input (T1, B, 32 F2), the last layer's output (T1, B, H))"""
    r = bf16_round if rounding else (lambda a: a)
    xin = rnn_input(mask_conv(p, x, rounding))
    h = xin
    for k in range(cfg["layers"]):
        h, _ = lstm_bidir(h, layer_of(p, k), rounding)
    logits = r(h) @ r(np.asarray(p["fc.module.weight"], np.float64)).T
    return logits, xin, h


def softmax_btc(logits):
    """PredictWithSoftmax: softmax over classes, (T1, B, C) -> (B, T1, C)."""
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).transpose(1, 0, 2)


@functools.lru_cache(maxsize=None)
def model_case(name, seed=0):
    """(cfg, state, x, exact logits, rounding-only logits) of SMALL / YAML_GEOMETRY, computed once per process."""
    cfg = {"small": SMALL, "yaml-geometry": YAML_GEOMETRY}[name]
    state, x = make_state(cfg, 11 + seed), make_input(cfg, 12 + seed, pad_frames=6)
    return cfg, state, x, forward(state, cfg, x)[0], forward(state, cfg, x, rounding=True)[0]


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def parse_audio(wave, sample_rate, window_size, window_stride, normalize):
    """dataset.py:31-48 in float64: stft with its default (hann) window, magnitude, log1p, whole-utterance normalisation (population
    standard deviation).  -> (features (F, frames), the magnitude before log1p)"""
    from oracle import speech_features as O

    n_fft, hop = int(sample_rate * window_size), int(sample_rate * window_stride)
    mag = np.abs(O.stft_vec(np.asarray(wave), n_fft=n_fft, hop_length=hop, win_length=n_fft).astype(np.complex128))
    feat = np.log1p(mag)
    if normalize:
        feat = (feat - feat.mean()) / feat.std()
    return feat, mag


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------
def greedy_string(frames, size, labels=LABELS):
    """process_string with remove_repetitions: drop blanks, drop a character equal to the previous FRAME's character, space -> ' '."""
    blank = labels.index("_")
    out = ""
    for i in range(int(size)):
        k = int(frames[i])
        if k == blank or (i > 0 and k == int(frames[i - 1])):
            continue
        out += labels[k]
    return out
