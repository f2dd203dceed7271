"""FastSpeech2 test cases without a device: a float64 restatement of `FastSpeech2.infer` (written from fastspeech2_v190.py:149-205,
variance_adapter.py and mindaudio/models/transformer/), the geometries the GPU tests run, and random weights with the reference's
initialisers.  Every row of the padded batch layout takes part, as in the reference.

`bf16_operands=True` rounds to bf16 exactly where the device does: both operands of every MFMA product (the operand image of the
residual stream, the weights, the fused QKV output, the attention probabilities and context, the FFN's hidden activation, the
predictors' normalised hidden activation).  Norms, residual adds, softmax statistics and the variance heads stay unrounded."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
PAD = 0


class H(dict):
    """A nested dict with attribute access: what the reference's yaml object looks like."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k)
        return H(v) if isinstance(v, dict) else v


def geometry(hidden, heads, layers, filt, conv_filter, n_bins, n_mels, max_seq_len, n_src_vocab=360):
    return H(use_fp16=False, n_mels=n_mels, hop_samples=300, n_fft=2048, sample_rate=22050,
             pitch=dict(feature="frame_level", normalization=False, pitch_min=0.0, pitch_max=843.436831),
             energy=dict(feature="frame_level", normalization=False, energy_min=0.0436493270, energy_max=494.149902),
             model=dict(n_src_vocab=n_src_vocab, max_seq_len=max_seq_len,
                        transformer=dict(encoder_layer=layers, encoder_head=heads, encoder_hidden=hidden, decoder_layer=layers,
                                         decoder_head=heads, decoder_hidden=hidden, conv_filter_size=conv_filter,
                                         conv_kernel_size=[9, 1], encoder_dropout=0.2, decoder_dropout=0.2),
                        variance_predictor=dict(filter_size=filt, kernel_size=3, dropout=0.5),
                        variance_embedding=dict(pitch_quantization="log", energy_quantization="linear", n_bins=n_bins)))


SMALL = geometry(64, 2, 1, 64, 128, 16, 16, 64, n_src_vocab=40)
YAML = geometry(256, 2, 1, 256, 1024, 256, 128, 1000)   # the shipped geometry with one layer per stack
YAML4 = geometry(256, 2, 4, 256, 1024, 256, 128, 1000)  # ... and as shipped


def sinusoid_closed_form(n_position, d_hid):
    """The table by its closed form, element by element (independent of the product's vectorised version)."""
    t = np.zeros((n_position, d_hid), np.float64)
    for pos in range(n_position):
        for j in range(d_hid):
            a = pos / (10000.0 ** (2 * (j // 2) / d_hid))
            t[pos, j] = math.sin(a) if j % 2 == 0 else math.cos(a)
    return t.astype(np.float32)


def bins_from_stats(hps):
    n = hps.model.variance_embedding.n_bins
    pitch = np.exp(np.linspace(np.log(hps.pitch.pitch_min + 1e-5), np.log(hps.pitch.pitch_max + 1e-5), n - 1)).astype(np.float32)
    energy = np.linspace(hps.energy.energy_min, hps.energy.energy_max, n - 1).astype(np.float32)
    return pitch, energy


def param_shapes(hps):
    """{state_dict name: shape} as the reference's cells define them (Conv1d weights (out, in, k))."""
    tr, vp = hps.model.transformer, hps.model.variance_predictor
    C, D, k, Fs, kv = tr.encoder_hidden, tr.conv_filter_size, tr.conv_kernel_size, vp.filter_size, vp.kernel_size
    n_bins, V = hps.model.variance_embedding.n_bins, hps.model.n_src_vocab + 1
    out = {}
    for stack, layers in (("expanded_encoder", tr.encoder_layer), ("encoder", tr.encoder_layer), ("decoder", tr.decoder_layer)):
        if stack != "decoder":
            out[stack + ".src_word_emb.weight"] = (V, C)
        for n in range(layers):
            p = "%s.layer_stack.%d." % (stack, n)
            for w in ("w_qs", "w_ks", "w_vs", "fc"):
                out[p + "slf_attn.%s.weight" % w], out[p + "slf_attn.%s.bias" % w] = (C, C), (C,)
            out[p + "slf_attn.layer_norm.gamma"], out[p + "slf_attn.layer_norm.beta"] = (C,), (C,)
            out[p + "pos_ffn.w_1.weight"], out[p + "pos_ffn.w_1.bias"] = (D, C, k[0]), (D,)
            out[p + "pos_ffn.w_2.weight"], out[p + "pos_ffn.w_2.bias"] = (C, D, k[1]), (C,)
            out[p + "pos_ffn.layer_norm.gamma"], out[p + "pos_ffn.layer_norm.beta"] = (C,), (C,)
    for pred in ("duration_predictor", "pitch_predictor", "energy_predictor"):
        p = "variance_adaptor.%s." % pred
        out[p + "conv1.0.weight"], out[p + "conv1.0.bias"] = (Fs, C, kv), (Fs,)
        out[p + "norm1.gamma"], out[p + "norm1.beta"] = (Fs,), (Fs,)
        out[p + "conv2.0.weight"], out[p + "conv2.0.bias"] = (Fs, Fs, kv), (Fs,)
        out[p + "norm2.gamma"], out[p + "norm2.beta"] = (Fs,), (Fs,)
        out[p + "linear_layer.weight"], out[p + "linear_layer.bias"] = (1, Fs), (1,)
    out["variance_adaptor.pitch_bins"], out["variance_adaptor.energy_bins"] = (n_bins - 1,), (n_bins - 1,)
    out["variance_adaptor.pitch_embedding.weight"], out["variance_adaptor.energy_embedding.weight"] = (n_bins, C), (n_bins, C)
    out["mel_linear.weight"], out["mel_linear.bias"] = (hps.n_mels, C), (hps.n_mels,)
    return out


def make_state(hps, seed, duration_bias=math.log(4.0)):
    """Random float32 weights with the reference's initialisers: Normal(0, sqrt(2 / (d_model + d_k))) for w_qs / w_ks / w_vs, MindSpore's
    default Normal(0, 0.01) for every other Dense / Conv1d / Embedding weight (the PAD row zero), zero biases, unit gamma, zero beta.
    Two departures that keep an untrained model testable: the norms' gamma / beta and the biases get a small random part (all-ones and
    all-zeros would hide a swapped or missing parameter), and the duration head's bias is log 4, so that predicted durations are
    round(exp(log 4 +- 0.2) - 1) = 2 .. 4 frames and the model expands."""
    g = torch.Generator().manual_seed(seed)
    C = hps.model.transformer.encoder_hidden
    d_k = C // hps.model.transformer.encoder_head
    state = {}
    for name, shape in param_shapes(hps).items():
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("_bins"):
            continue
        if leaf == "gamma":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif leaf in ("beta", "bias"):
            t = 0.05 * torch.randn(shape, generator=g)
        else:
            sigma = math.sqrt(2.0 / (C + d_k)) if any(w in name for w in (".w_qs.", ".w_ks.", ".w_vs.")) else 0.01
            t = sigma * torch.randn(shape, generator=g)
            if name.endswith("src_word_emb.weight"):
                t[PAD] = 0.0
        state[name] = t.to(torch.float32)
    state["variance_adaptor.duration_predictor.linear_layer.bias"] = torch.tensor([duration_bias], dtype=torch.float32)
    pb, eb = bins_from_stats(hps)
    state["variance_adaptor.pitch_bins"], state["variance_adaptor.energy_bins"] = torch.from_numpy(pb), torch.from_numpy(eb)
    return state


def make_inputs(hps, src_lens, seed):
    """texts (B, max(src_lens)) int64 with ids 1 .. n_src_vocab inside each utterance and PAD beyond it."""
    rng = np.random.default_rng(seed)
    Ts = max(src_lens)
    texts = np.zeros((len(src_lens), Ts), np.int64)
    for b, n in enumerate(src_lens):
        texts[b, :n] = rng.integers(1, hps.model.n_src_vocab + 1, size=n)
    return texts, np.asarray(src_lens, np.int64)


def rb(x, on):
    """Round to bf16 (nearest even) and back, when `on`."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64) if on else x


def masked_softmax(s, key_mask):
    """softmax over the last axis with masked keys at -inf (score_function.py:25-30); a row with every key masked gives zeros (the
    stated departure: the reference gives NaN)."""
    s = s.masked_fill(key_mask, -math.inf)
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m).masked_fill(key_mask, 0.0)
    return e, e.sum(-1, keepdim=True)


def group_norm(x, groups, gamma, beta, eps=1e-5):
    """GroupNorm(groups, C) of the (B, C, T, 1) view of x (B, T, C): statistics over all T rows x C / groups channels, biased variance."""
    B, T, C = x.shape
    v = x.reshape(B, T, groups, C // groups)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    return ((v - mean) / torch.sqrt(var + eps)).reshape(B, T, C) * gamma + beta


def layer_norm(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def conv_same(x, w, b, bf):
    """nn.Conv1d(pad_mode="same", odd kernel) on x (B, T, C) with w (out, in, k)."""
    k = w.shape[-1]
    return F.conv1d(rb(x, bf).transpose(1, 2), rb(w, bf), b, padding=k // 2).transpose(1, 2)


def fft_block(x, st, p, n_head, key_mask, norm, bf):
    """FFTBlock (layers.py:27-34): x (B, T, C), key_mask (B, T) True at masked positions."""
    B, T, C = x.shape
    d_k = C // n_head
    w = lambda n: st[p + n].to(F64)
    nrm = (lambda y, pre: group_norm(y, 8, w(pre + ".gamma"), w(pre + ".beta"))) if norm == "group" else \
        (lambda y, pre: layer_norm(y, w(pre + ".gamma"), w(pre + ".beta"), 1e-5))
    keep = (~key_mask).to(F64)[:, :, None]
    xin = rb(x, bf)
    q, k, v = (rb(xin @ rb(w("slf_attn.%s.weight" % n), bf).T + w("slf_attn.%s.bias" % n), bf).reshape(B, T, n_head, d_k).transpose(1, 2)
               for n in ("w_qs", "w_ks", "w_vs"))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(d_k)
    e, _ = masked_softmax(s, key_mask[:, None, None, :])
    e = rb(e, bf)
    l = e.sum(-1, keepdim=True)
    ctx = (e @ v) / torch.where(l > 0, l, torch.ones_like(l))
    ctx = rb(ctx.transpose(1, 2).reshape(B, T, C), bf)
    y = ctx @ rb(w("slf_attn.fc.weight"), bf).T + w("slf_attn.fc.bias") + x
    x = nrm(y, "slf_attn.layer_norm") * keep
    hid = rb(torch.relu(conv_same(x, w("pos_ffn.w_1.weight"), w("pos_ffn.w_1.bias"), bf)), bf)
    y = conv_same(hid, w("pos_ffn.w_2.weight"), w("pos_ffn.w_2.bias"), bf) + x
    return nrm(y, "pos_ffn.layer_norm") * keep


def variance_predictor(x, st, p, mask, bf):
    """VariancePredictor (variance_adapter.py:71-89) -> (B, T); LayerNorm eps 1e-7 (MindSpore's default)."""
    w = lambda n: st[p + n].to(F64)
    hcur = torch.relu(conv_same(x, w("conv1.0.weight"), w("conv1.0.bias"), bf))
    hcur = layer_norm(hcur, w("norm1.gamma"), w("norm1.beta"), 1e-7)
    hcur = torch.relu(conv_same(hcur, w("conv2.0.weight"), w("conv2.0.bias"), bf))
    hcur = layer_norm(hcur, w("norm2.gamma"), w("norm2.beta"), 1e-7)
    out = (hcur @ w("linear_layer.weight").T + w("linear_layer.bias"))[..., 0]
    if mask is not None:
        out = out * (~mask).to(F64)
    return out


def round_durations(logd, d_control):
    """round(exp(logd) - 1) * d_control clipped at 0, in float32 as the reference computes it: exp correctly rounded (through float64),
    one float32 subtraction, round half to even, one float32 product."""
    e = np.exp(np.asarray(logd, np.float64)).astype(np.float32)
    r = np.rint(e - np.float32(1.0)).astype(np.float32)
    return np.maximum(r * np.float32(d_control), np.float32(0.0)).astype(np.float32)


def length_regulate(ids, durations):
    """LengthRegulator on token ids (variance_adapter.py:12-31): np.repeat per row, padded with 0 to the longest."""
    rows = [np.repeat(np.asarray(r), np.asarray(d).astype(np.int32)) for r, d in zip(ids, durations)]
    mel_len = np.asarray([len(r) for r in rows], np.int64)
    out = np.zeros((len(rows), int(mel_len.max()) if len(rows) else 0), np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, mel_len


def infer(hps, state, texts, src_lens, p_control=1.0, e_control=1.0, d_control=1.0, norm="group", bf16_operands=False, overrides=None):
    """The restatement.  -> dict of float64 / integer NumPy arrays with the model's keys (all rows)."""
    ov, bf = dict(overrides or {}), bf16_operands
    st = state
    tr = hps.model.transformer
    C = tr.encoder_hidden
    texts = np.asarray(texts, np.int64)
    B, Ts = texts.shape
    pos = torch.from_numpy(sinusoid_closed_form(hps.model.max_seq_len + 1, C)).to(F64)

    def encoder(name, ids, n_head):
        idt = torch.from_numpy(ids)
        x = st[name + ".src_word_emb.weight"].to(F64)[idt] + pos[None, :ids.shape[1]]
        x = x.to(torch.float32).to(F64)  # the stream is float32 on the device: one rounding here keeps the bf16 image identical
        key_mask = idt == PAD
        for n in range(tr.encoder_layer):
            x = fft_block(x, st, "%s.layer_stack.%d." % (name, n), n_head, key_mask, norm, bf)
        return x

    src_mask = torch.from_numpy(np.arange(Ts)[None, :] >= np.asarray(src_lens)[:, None])
    x = encoder("encoder", texts, tr.encoder_head)
    logd = variance_predictor(x, st, "variance_adaptor.duration_predictor.", src_mask, bf)
    dur = np.asarray(ov["durations"], np.float32) if "durations" in ov else round_durations(logd.numpy().astype(np.float32), d_control)
    ids_exp, mel_len = length_regulate(texts, dur)
    T = ids_exp.shape[1]
    if T > hps.model.max_seq_len + 1:
        raise ValueError("mel longer than max_seq_len + 1")
    mel_mask = torch.from_numpy(np.arange(T)[None, :] >= mel_len[:, None])
    x = encoder("expanded_encoder", ids_exp, tr.encoder_head)
    pbins, ebins = st["variance_adaptor.pitch_bins"].numpy(), st["variance_adaptor.energy_bins"].numpy()
    pitch = variance_predictor(x, st, "variance_adaptor.pitch_predictor.", None, bf) * p_control
    pidx = np.asarray(ov["pitch_index"], np.int64) if "pitch_index" in ov else np.searchsorted(pbins, pitch.numpy().astype(np.float32), "left")
    x = x + st["variance_adaptor.pitch_embedding.weight"].to(F64)[torch.from_numpy(pidx)]
    energy = variance_predictor(x, st, "variance_adaptor.energy_predictor.", None, bf) * e_control
    eidx = np.asarray(ov["energy_index"], np.int64) if "energy_index" in ov else np.searchsorted(ebins, energy.numpy().astype(np.float32), "left")
    x = x + st["variance_adaptor.energy_embedding.weight"].to(F64)[torch.from_numpy(eidx)]
    output = x
    x = x + pos[None, :T]
    for n in range(tr.decoder_layer):
        x = fft_block(x, st, "decoder.layer_stack.%d." % n, tr.decoder_head, mel_mask, norm, bf)
    mel = rb(x, bf) @ rb(st["mel_linear.weight"].to(F64), bf).T + st["mel_linear.bias"].to(F64)
    return {"output": output.numpy(), "pitch_predictions": pitch.numpy(), "energy_predictions": energy.numpy(),
            "log_duration_predictions": logd.numpy(), "duration_rounded": dur, "mel_len": mel_len, "mel_masks": mel_mask.numpy(),
            "mel_predictions": mel.numpy(), "src_masks": src_mask.numpy(), "pitch_index": pidx, "energy_index": eidx,
            "exp_minus_one": np.exp(logd.numpy()) - 1.0}


def relrms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-300))
