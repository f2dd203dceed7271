"""The float64 NumPy restatement of TasNet (mindaudio/models/tasnet.py, mindaudio/loss/separation_loss.py:13-130) that
test_tasnet_cpu.py / test_tasnet_gpu.py measure against, in the reference's own layouts: mixture (B, K, L), Conv1d weights (N, L, 1),
est_source (B, nspk, K, L).  The LSTM cell is deepspeech2_cases.lstm_direction.

Two forms of every stage:
  exact         float64 throughout.
  rounding-only the same float64 arithmetic with values rounded to bf16 (through float32, round to nearest even) at exactly the
                points where the device rounds: the LayerNorm output; in every LSTM layer x, W_ih, W_hh and the h that is fed back
                (the h handed to the next layer is that layer's x); the fc input and weight.  mixture_w, norm_coef, gate sums, c, the
                softmax and the decoder are never rounded.
S = relrms(rounding-only, exact) is the yardstick; the device tests allow 2 S, the factor covering float32 accumulation order and
float32 sigmoid / tanh / exp, which the rounding-only form lacks.  No figure here is measured on the code under test."""
import functools
import json
import os

import numpy as np

from deepspeech2_cases import bf16_round, lstm_direction, relrms, sigmoid  # noqa: F401

EPS = 1e-8
LN_EPS = 1e-7  # mindspore.nn.LayerNorm's default epsilon

SMALL = dict(L=8, N=40, H=64, layers=4, nspk=2, B=3, K=19)
TINY = dict(L=8, N=40, H=64, layers=4, nspk=2, B=2, K=2)
YAML_GEOMETRY = dict(L=40, N=500, H=512, layers=4, nspk=2, B=1, K=12)
CASES = {"small": SMALL, "tiny": TINY, "yaml-geometry": YAML_GEOMETRY}
FC_GAIN = 32.0  # at plain Xavier gain the masks sit near 0.5 and S falls to 1e-5, too close to float32 accumulation


# ---- LSTM stack -------------------------------------------------------------------------------------------------------------------------
def stack_params(seed, K, H, layers):
    """uniform(+-1 / sqrt(H)) float32 per layer: [{weight_ih (4H, K_l), weight_hh (4H, H), bias_ih, bias_hh}]."""
    g = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(H)
    return [{n: g.uniform(-k, k, s).astype(np.float32) for n, s in
             (("weight_ih", (4 * H, K if l == 0 else H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,)))}
            for l in range(layers)]


def lstm_stack(x, layers, rounding=False, stats=None):
    """nn.LSTM(num_layers=len(layers), bidirectional=False) on x (T, B, K), h0 = c0 = 0 -> (out (T, B, H) of the last layer,
    h_final (layers, B, H), c_final (layers, B, H)).  stats: a list that receives one list of min |gate| per step for every layer."""
    h = np.asarray(x, np.float64)
    hs, cs = [], []
    for p in layers:
        st = [] if stats is not None else None
        h, c = lstm_direction(h, p["weight_ih"], p["weight_hh"], p["bias_ih"], p["bias_hh"], False, rounding, st)
        if stats is not None:
            stats.append(st)
        hs.append(h[-1])
        cs.append(c)
    return h, np.stack(hs), np.stack(cs)


def stack_routing_case(T, B, H, layers, K=64, seed=0):
    """deepspeech2_cases.routing_case carried through a stack: every gate of every layer is saturated, so that h and c move in steps
    of the saturated cell and a layer fed from the wrong parity image, a wrong layer's weights, an off-by-one diagonal, a swapped gate
    or a wrong batch row changes the result by O(1).  gate = a + b + r with
      a  layer 0: x[t, b] is one-hot at column (3 t + 5 b + 1) % K and W_ih is 0 or +-128 -> a in {0, +-128};
         layer l >= 1: ONE non-zero W_ih entry per gate row, +-256, at a column that depends on the layer, the gate and the unit;
         its operand is the lower layer's h with |h| = sigmoid(o) |tanh(c)|, c an integer up to the saturation residue, so
         |h| is 0 or in [tanh(1), 1] = [0.7616, 1] and a is 0 or in +-[194.9, 256];
      b  bias_ih = +-32, bias_hh = 0;
      r  ONE non-zero W_hh entry per gate row, +-64: r is 0 or in +-[48.7, 64].
    Whatever the signs, |a + b + r| >= 16.7: for layer 0 as in routing_case; above it |+-a +- r| is 0, in [48.7, 64] or >= 130.9, each
    at least 16.7 away from 32.  (+-128 in the upper layers' W_ih, as in layer 0, would not do: 128 tanh(1) - 64 - 32 = 1.5.)
    The weights are exact in bf16; the fed-back and handed-up h are not, but their rounding (2^-9 relative) moves a gate by at most
    0.5, which leaves it saturated: 1 - sigmoid(16.2) = 9.2e-8.  The float64 restatement and a correct float32 kernel therefore differ
    by saturation residues and float32 roundings of c accumulated over T <= 7 steps, below the bound 1e-6.
    The patterns differ per layer, per gate row (hence per hidden slice) and per batch row (through x)."""
    g = np.random.RandomState(2000 + seed + 7 * T + 13 * B + H + 31 * layers)
    x = np.zeros((T, B, K), np.float32)
    for t in range(T):
        for b in range(B):
            x[t, b, (3 * t + 5 * b + 1) % K] = 1.0
    out = []
    for l in range(layers):
        if l == 0:
            w_ih = (g.randint(-1, 2, (4 * H, K)) * 128).astype(np.float32)
        else:
            w_ih = np.zeros((4 * H, H), np.float32)
            for gate in range(4):
                for j in range(H):
                    w_ih[gate * H + j, (5 * j + 1 + 3 * gate + 11 * l) % H] = g.choice([-256.0, 256.0])
        w_hh = np.zeros((4 * H, H), np.float32)
        for gate in range(4):
            for j in range(H):
                w_hh[gate * H + j, (7 * j + 3 + gate + 5 * l) % H] = g.choice([-64.0, 64.0])
        b_ih = g.choice([-32.0, 32.0], (4 * H,)).astype(np.float32)
        out.append(dict(weight_ih=w_ih, weight_hh=w_hh, bias_ih=b_ih, bias_hh=np.zeros_like(b_ih)))
    return x, out


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def param_shapes(L, N, H, layers, nspk=2, **_):
    out = {}
    for c in ("U", "V"):
        out["encoder.conv1d_%s.weight" % c] = (N, L, 1)
        out["encoder.conv1d_%s.bias" % c] = (N,)
    out["separator.layer_norm.gamma"] = out["separator.layer_norm.beta"] = (N,)
    for l in range(layers):
        out["separator.lstm.weight_ih_l%d" % l] = (4 * H, N if l == 0 else H)
        out["separator.lstm.weight_hh_l%d" % l] = (4 * H, H)
        out["separator.lstm.bias_ih_l%d" % l] = out["separator.lstm.bias_hh_l%d" % l] = (4 * H,)
    out["separator.fc.weight"], out["separator.fc.bias"] = (nspk * N, H), (nspk * N,)
    out["decoder.basis_signals.weight"], out["decoder.basis_signals.bias"] = (L, N), (L,)
    return out


def make_state(cfg, seed, fc_gain=FC_GAIN):
    """Seeded float32 weights: Xavier-uniform Conv1d / Dense weights as the reference initialises them (the fc weight at fc_gain times
    that), biases uniform(+-0.1), LayerNorm gamma / beta away from the identity, LSTM uniform(+-1 / sqrt(H))."""
    g = np.random.RandomState(seed)
    state = {}
    for name, shape in param_shapes(**cfg).items():
        leaf = name.rsplit(".", 1)[1]
        if ".lstm." in name:
            v = g.uniform(-1.0, 1.0, shape) / np.sqrt(cfg["H"])
        elif leaf == "gamma":
            v = g.uniform(0.8, 1.2, shape)
        elif leaf == "beta":
            v = g.uniform(-0.2, 0.2, shape)
        elif leaf == "bias":
            v = g.uniform(-0.1, 0.1, shape)
        else:
            bound = np.sqrt(6.0 / (shape[0] + shape[1])) * (fc_gain if name == "separator.fc.weight" else 1.0)
            v = g.uniform(-bound, bound, shape)
        state[name] = v.astype(np.float32)
    return state


def make_mixture(cfg, seed, zero_last=False):
    """(B, K, L) float32 'waveform segments'; zero_last: the last segment of the last row is all zero, like the eval padding."""
    x = (0.1 * np.random.RandomState(seed).normal(0.0, 1.0, (cfg["B"], cfg["K"], cfg["L"]))).astype(np.float32)
    if zero_last:
        x[-1, -1] = 0.0
    return x


def layers_of(p, n):
    return [{k: np.asarray(p["separator.lstm.%s_l%d" % (k, l)]) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
            for l in range(n)]


def encoder(p, mixture, rounding=False):
    """tasnet.py:72-90 and the separator's LayerNorm (:123) -> (mixture_w (B, K, N), norm_coef (B, K), normalised (B, K, N))."""
    r = bf16_round if rounding else (lambda a: a)
    f = lambda k: np.asarray(p[k], np.float64)  # noqa: E731
    x = np.asarray(mixture, np.float64)
    norm = np.sqrt((x ** 2).sum(2))
    xn = x / (norm[..., None] + EPS)
    u = xn @ f("encoder.conv1d_U.weight")[:, :, 0].T + f("encoder.conv1d_U.bias")
    v = xn @ f("encoder.conv1d_V.weight")[:, :, 0].T + f("encoder.conv1d_V.bias")
    w = np.maximum(u, 0.0) * sigmoid(v)
    mean = w.mean(2, keepdims=True)
    var = ((w - mean) ** 2).mean(2, keepdims=True)
    ln = (w - mean) / np.sqrt(var + LN_EPS) * f("separator.layer_norm.gamma") + f("separator.layer_norm.beta")
    return w, norm, r(ln)


def mask_decode(p, score, mixture_w, norm_coef, nspk):
    """tasnet.py:130-165: score (B, K, nspk * N) -> est_source (B, nspk, K, L)."""
    B, K, N = mixture_w.shape
    s = np.asarray(score, np.float64).reshape(B, K, nspk, N)
    e = np.exp(s - s.max(2, keepdims=True))
    mask = e / e.sum(2, keepdims=True)
    source_w = np.asarray(mixture_w, np.float64)[:, :, None, :] * mask
    est = source_w @ np.asarray(p["decoder.basis_signals.weight"], np.float64).T + np.asarray(p["decoder.basis_signals.bias"], np.float64)
    return (est * np.asarray(norm_coef, np.float64)[:, :, None, None]).transpose(0, 2, 1, 3)


def forward(p, cfg, mixture, rounding=False):
    """-> (est_source (B, nspk, K, L), the LSTM stack's output (K, B, H))"""
    r = bf16_round if rounding else (lambda a: a)
    w, norm, ln = encoder(p, mixture, rounding)
    h, _, _ = lstm_stack(ln.transpose(1, 0, 2), layers_of(p, cfg["layers"]), rounding)
    score = r(h) @ r(np.asarray(p["separator.fc.weight"], np.float64)).T + np.asarray(p["separator.fc.bias"], np.float64)
    return mask_decode(p, score.transpose(1, 0, 2), w, norm, cfg["nspk"]), h


@functools.lru_cache(maxsize=None)
def model_case(name, seed=0):
    """(cfg, state, mixture, exact est_source, rounding-only est_source, exact stack output, rounding-only stack output), once per
    process."""
    cfg = CASES[name]
    state, x = make_state(cfg, 21 + seed), make_mixture(cfg, 22 + seed, zero_last=True)
    exact, h = forward(state, cfg, x)
    rounded, hr = forward(state, cfg, x, rounding=True)
    return cfg, state, x, exact, rounded, h, hr


@functools.lru_cache(maxsize=None)
def stack_case(T, B, H, K, layers):
    """(x (T, B, K) bf16-valued, layer parameters, exact (out, h_final, c_final), rounding-only (out, h_final, c_final)) of a
    random-weight stack."""
    p = stack_params(300 + K + H + layers, K, H, layers)
    x = bf16_round(np.random.RandomState(T * 31 + B).normal(0, 1, (T, B, K)))  # a bf16 activation, as the encoder leaves it
    exact = lstm_stack(x, p)
    return x, p, exact, lstm_stack(x, p, rounding=True)


# ---- Separation_Loss --------------------------------------------------------------------------------------------------------------------
def separation_loss(source, estimate, lengths):
    """separation_loss.py:40-130 for [B, 2, K, L] in float64, unmasked: -> (loss, max_snr (B, 1), perm (B, 2), reordered)."""
    s, e = np.asarray(source, np.float64), np.asarray(estimate, np.float64)
    B, C, K, L = s.shape
    n = (L * np.asarray(lengths, np.float64)).reshape(B, 1, 1)
    fs, fe = s.reshape(B, C, -1), e.reshape(B, C, -1)
    fs, fe = fs - fs.sum(2, keepdims=True) / n, fe - fe.sum(2, keepdims=True) / n
    pair = np.zeros((B, C, C))
    for b in range(B):
        for i in range(C):      # estimate
            for j in range(C):  # target
                t = fs[b, j]
                proj = (fe[b, i] @ t) * t / (t @ t + EPS)
                noise = fe[b, i] - proj
                pair[b, i, j] = 10 * np.log10((proj @ proj) / (noise @ noise + EPS) + EPS)
    keep, swap = pair[:, 0, 0] + pair[:, 1, 1], pair[:, 0, 1] + pair[:, 1, 0]
    swapped = swap > keep
    max_snr = (np.where(swapped, swap, keep) / C).reshape(B, 1)
    perm = np.where(swapped[:, None], np.array([[1, 0]]), np.array([[0, 1]]))
    reordered = np.stack([e[b, perm[b]] for b in range(B)])
    return -max_snr.mean(), max_snr, perm, reordered


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def write_dataset(root, lengths, names, rate=8000, seed=0):
    """Three tiny utterances as mix / s1 / s2 wav files and their json lists (in file order, NOT sorted); -> {name: (mix, s1, s2)}."""
    from scipy.io import wavfile

    g = np.random.RandomState(seed)
    waves, lists = {}, {"mix_clean": [], "s1": [], "s2": []}
    for n, name in zip(lengths, names):
        s1, s2 = (np.round(0.2 * g.normal(0, 1, n) * 32767).clip(-32767, 32767).astype(np.int16) for _ in range(2))
        mix = ((s1.astype(np.int32) + s2) // 2).astype(np.int16)
        waves[name] = tuple(a.astype(np.float32) / 32768.0 for a in (mix, s1, s2))
        for key, a in (("mix_clean", mix), ("s1", s1), ("s2", s2)):
            os.makedirs(os.path.join(root, key), exist_ok=True)
            path = os.path.join(root, key, name + ".wav")
            wavfile.write(path, rate, a)
            lists[key].append([path, int(n)])
    for key, entries in lists.items():
        with open(os.path.join(root, key + ".json"), "w") as fh:
            json.dump(entries, fh)
    return waves
