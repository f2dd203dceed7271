"""FastSpeech2 on MI355X - mirror of mindaudio.models.fastspeech2.FastSpeech2 (fastspeech2_v190.py:10-205), `infer` only.

The residual stream is time-major, channel-last float32; bf16 exists only as the MFMA operand image (B, T + 2 halo, C) with zero halo rows.
The dense layers and convolutions are ma_gemm_bf16 / ma_conv1d_taps_bf16; csrc/fastspeech2.hip holds the rest (the masked attention, the
GroupNorm pair, the row LayerNorm, the variance head, the embedding, the duration rule and the length regulator).  Each of the three
FFT-block stacks is one C call (ma_fs2_fft_stack).  One `infer` reads back exactly one thing from the device: mel_len (B integers), which
sizes the frame-level buffers.

PyTorch layers are parameter containers (their forward() is never called), named as the reference's cells: encoder / expanded_encoder
.src_word_emb, {encoder, expanded_encoder, decoder}.layer_stack.<n>.{slf_attn.{w_qs, w_ks, w_vs, fc, layer_norm}, pos_ffn.{w_1, w_2,
layer_norm}}, variance_adaptor.{duration, pitch, energy}_predictor.{conv1.0, norm1, conv2.0, norm2, linear_layer},
variance_adaptor.{pitch_bins, energy_bins, pitch_embedding, energy_embedding}, mel_linear."""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _host, _lib
from .wavegrad import _get

__all__ = ["FastSpeech2", "sinusoid_table", "variance_bins"]

PAD = 0  # transformer/constants.py
_LN_EPS = 1e-7  # MindSpore's nn.LayerNorm default (the VariancePredictor norms)
_NORM_EPS = 1e-5  # nn.GroupNorm's default, used for both block norms


def sinusoid_table(n_position, d_hid):
    """get_sinusoid_encoding_table (transformer/positional_encoding.py:4-21): float64 arithmetic, rounded to float32."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)
    ang = pos / np.power(10000.0, 2.0 * (j // 2) / d_hid)[None, :]
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return ang.astype(np.float32)


def variance_bins(stats, n_bins, pitch_quantization="log", energy_quantization="linear"):
    """The n_bins - 1 float32 bin edges of variance_adapter.py:114-143 from stats = (pitch_min, pitch_max, energy_min, energy_max)."""
    pmin, pmax, emin, emax = (float(v) for v in stats)
    if pitch_quantization == "log":
        pitch = np.exp(np.linspace(np.log(pmin + 1e-5), np.log(pmax + 1e-5), n_bins - 1))
    else:
        pitch = np.linspace(pmin, pmax, n_bins - 1)
    if energy_quantization == "log":
        energy = np.exp(np.linspace(np.log(emin), np.log(emax), n_bins - 1))
    else:
        energy = np.linspace(emin, emax, n_bins - 1)
    return pitch.astype(np.float32), energy.astype(np.float32)


class _Norm(nn.Module):
    """gamma / beta of nn.GroupNorm or nn.LayerNorm: the parameter names are the same for both."""

    def __init__(self, c):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(c))
        self.beta = nn.Parameter(torch.zeros(c))


def _dense(cin, cout, sigma=0.01):
    lin = nn.Linear(cin, cout)
    nn.init.normal_(lin.weight, 0.0, sigma)  # MindSpore's Dense: weight "normal" (sigma 0.01) unless given, bias zeros
    nn.init.zeros_(lin.bias)
    return lin


def _conv(cin, cout, k):
    conv = nn.Conv1d(cin, cout, k)
    nn.init.normal_(conv.weight, 0.0, 0.01)
    nn.init.zeros_(conv.bias)
    return conv


class _MHA(nn.Module):
    def __init__(self, d_model, n_head, d_k):
        super().__init__()
        sigma = math.sqrt(2.0 / (d_model + d_k))  # sublayers.py:17-45
        self.w_qs, self.w_ks, self.w_vs = (_dense(d_model, n_head * d_k, sigma) for _ in range(3))
        self.fc = _dense(n_head * d_k, d_model, 0.01)
        self.layer_norm = _Norm(d_model)


class _FFN(nn.Module):
    def __init__(self, d_in, d_hid, kernels):
        super().__init__()
        self.w_1, self.w_2 = _conv(d_in, d_hid, kernels[0]), _conv(d_hid, d_in, kernels[1])
        self.layer_norm = _Norm(d_in)


class _FFTBlock(nn.Module):
    def __init__(self, d_model, d_inner, kernels, n_head):
        super().__init__()
        self.slf_attn, self.pos_ffn = _MHA(d_model, n_head, d_model // n_head), _FFN(d_model, d_inner, kernels)


class _Stack(nn.Module):
    def __init__(self, d_model, d_inner, kernels, n_head, n_layers, n_vocab=None):
        super().__init__()
        if n_vocab is not None:
            self.src_word_emb = nn.Embedding(n_vocab, d_model, padding_idx=PAD)
            nn.init.normal_(self.src_word_emb.weight, 0.0, 0.01)
            with torch.no_grad():
                self.src_word_emb.weight[PAD].zero_()
        self.layer_stack = nn.ModuleList([_FFTBlock(d_model, d_inner, kernels, n_head) for _ in range(n_layers)])
        self.n_head = n_head


class _VariancePredictor(nn.Module):
    def __init__(self, cin, filt, k):
        super().__init__()
        self.conv1, self.norm1 = nn.Sequential(_conv(cin, filt, k), nn.ReLU()), _Norm(filt)
        self.conv2, self.norm2 = nn.Sequential(_conv(filt, filt, k), nn.ReLU()), _Norm(filt)
        self.linear_layer = _dense(filt, 1)


class _VarianceAdaptor(nn.Module):
    def __init__(self, hidden, filt, k, n_bins, pitch_bins, energy_bins):
        super().__init__()
        self.duration_predictor = _VariancePredictor(hidden, filt, k)
        self.pitch_predictor = _VariancePredictor(hidden, filt, k)
        self.energy_predictor = _VariancePredictor(hidden, filt, k)
        self.register_buffer("pitch_bins", torch.from_numpy(pitch_bins))
        self.register_buffer("energy_bins", torch.from_numpy(energy_bins))
        self.pitch_embedding, self.energy_embedding = nn.Embedding(n_bins, hidden), nn.Embedding(n_bins, hidden)
        nn.init.normal_(self.pitch_embedding.weight, 0.0, 0.01)
        nn.init.normal_(self.energy_embedding.weight, 0.0, 0.01)


class FastSpeech2(nn.Module):
    """FastSpeech2(hps, stats=None, norm="group"): hps is the object with the attributes of fastspeech2.yaml, or a nested dict.

    stats = (pitch_min, pitch_max, energy_min, energy_max) replaces the reference's np.load("stats.npy") from the working directory;
    None takes hps.pitch.pitch_min / pitch_max and hps.energy.energy_min / energy_max.  norm = "group" (default) reads the reference's
    nn.GroupNorm([8, d_model]) as 8 groups over d_model channels; norm = "layer" is its commented-out LayerNorm([d_model]).

    Not built (NotImplementedError): use_fp16, forward / forward_expanded / construct (the training paths), phoneme-level pitch or
    energy, a second FFN kernel other than 1, even kernels, widths that are no multiples of 64, a head size outside {32, 64, 128}."""

    def __init__(self, hps, stats=None, norm="group"):
        super().__init__()
        if _get(hps, "use_fp16"):
            raise NotImplementedError("use_fp16: the float16 cells are not built (activations are float32, operands bf16)")
        if norm not in ("group", "layer"):
            raise ValueError("norm must be 'group' or 'layer'")
        model, tr = _get(hps, "model"), _get(_get(hps, "model"), "transformer")
        vp, ve = _get(model, "variance_predictor"), _get(model, "variance_embedding")
        pitch, energy = _get(hps, "pitch"), _get(hps, "energy")
        if _get(pitch, "feature") != "frame_level" or _get(energy, "feature") != "frame_level":
            raise NotImplementedError("phoneme_level pitch / energy features are not built (infer adds them at frame level)")
        hidden = int(_get(tr, "encoder_hidden"))
        if int(_get(tr, "decoder_hidden")) != hidden:
            raise NotImplementedError("decoder_hidden must equal encoder_hidden (the adaptor's output feeds the decoder as it is)")
        d_inner, kernels = int(_get(tr, "conv_filter_size")), [int(k) for k in _get(tr, "conv_kernel_size")]
        filt, vk = int(_get(vp, "filter_size")), int(_get(vp, "kernel_size"))
        heads = (int(_get(tr, "encoder_head")), int(_get(tr, "decoder_head")))
        if kernels[1] != 1 or kernels[0] % 2 == 0 or vk % 2 == 0:
            raise NotImplementedError("built for conv_kernel_size [odd, 1] and an odd variance_predictor.kernel_size")
        if hidden % 64 or d_inner % 64 or filt % 64 or hidden > 1024 or filt > 1024:
            raise NotImplementedError("hidden, conv_filter_size and filter_size must be multiples of 64 (hidden, filter_size <= 1024)")
        if any(hidden % h or hidden // h not in (32, 64, 128) for h in heads):
            raise NotImplementedError("the attention kernel is built for d_k in {32, 64, 128}")
        self.groups = 8 if norm == "group" else 0
        if self.groups and (hidden % 8 or (hidden // 8) % 4):
            raise NotImplementedError("GroupNorm(8, hidden) needs hidden / 8 to be a multiple of 4")
        self.hidden, self.d_inner, self.kernels, self.filter, self.vk = hidden, d_inner, kernels, filt, vk
        self.n_mels, self.n_bins = int(_get(hps, "n_mels")), int(_get(ve, "n_bins"))
        self.max_seq_len = int(_get(model, "max_seq_len"))
        self.halo = max(kernels[0] // 2, vk // 2)
        n_vocab = int(_get(model, "n_src_vocab")) + 1
        if stats is None:
            stats = (_get(pitch, "pitch_min"), _get(pitch, "pitch_max"), _get(energy, "energy_min"), _get(energy, "energy_max"))
        pb, eb = variance_bins(stats, self.n_bins, _get(ve, "pitch_quantization"), _get(ve, "energy_quantization"))
        self.expanded_encoder = _Stack(hidden, d_inner, kernels, heads[0], int(_get(tr, "encoder_layer")), n_vocab)
        self.encoder = _Stack(hidden, d_inner, kernels, heads[0], int(_get(tr, "encoder_layer")), n_vocab)
        self.variance_adaptor = _VarianceAdaptor(hidden, filt, vk, self.n_bins, pb, eb)
        self.decoder = _Stack(hidden, d_inner, kernels, heads[1], int(_get(tr, "decoder_layer")))
        self.mel_linear = _dense(hidden, self.n_mels)
        self.speaker_emb = None  # fastspeech2_v190.py:21
        self.register_buffer("position_enc", torch.from_numpy(sinusoid_table(self.max_seq_len + 1, hidden)), persistent=False)
        self._prepared = None
        self.register_load_state_dict_post_hook(lambda module, _keys: module._drop())
        self.launches = 0  # kernel launches of the last infer()

    def _drop(self):
        self._prepared = None

    def forward(self, *args, **kwargs):
        raise NotImplementedError("FastSpeech2.forward (the teacher-forced training path) is not built; use infer()")

    def forward_expanded(self, *args, **kwargs):
        raise NotImplementedError("FastSpeech2.forward_expanded (the training path behind construct) is not built; use infer()")

    construct = forward_expanded

    # ---- weights ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self):
        """The operand copies: dense weights (out, in) bf16 (w_qs | w_ks | w_vs stacked), Conv1d weights (out, in, k) -> (out, k, in)
        bf16, everything else float32 contiguous."""
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        bf = lambda t: t.detach().to(torch.float32).to(torch.bfloat16).contiguous()
        cw = lambda conv: bf(conv.weight.permute(0, 2, 1))
        P = {}
        for name in ("encoder", "expanded_encoder", "decoder"):
            stack, layers = getattr(self, name), []
            for blk in stack.layer_stack:
                a, f = blk.slf_attn, blk.pos_ffn
                layers.append(dict(
                    w_qkv=bf(torch.cat([a.w_qs.weight, a.w_ks.weight, a.w_vs.weight], 0)),
                    b_qkv=f32(torch.cat([a.w_qs.bias, a.w_ks.bias, a.w_vs.bias], 0)), w_fc=bf(a.fc.weight), b_fc=f32(a.fc.bias),
                    gamma1=f32(a.layer_norm.gamma), beta1=f32(a.layer_norm.beta), w_1=cw(f.w_1), b_1=f32(f.w_1.bias),
                    w_2=bf(f.w_2.weight[:, :, 0]), b_2=f32(f.w_2.bias), gamma2=f32(f.layer_norm.gamma), beta2=f32(f.layer_norm.beta)))
            arr = (_lib.Fs2Layer * len(layers))()
            for o, d in zip(arr, layers):
                for k, v in d.items():
                    setattr(o, k, v.data_ptr())
            P[name] = (arr, layers)
            if hasattr(stack, "src_word_emb"):
                P[name + ".emb"] = f32(stack.src_word_emb.weight)
        va = self.variance_adaptor
        for name in ("duration_predictor", "pitch_predictor", "energy_predictor"):
            p = getattr(va, name)
            P[name] = dict(w1=cw(p.conv1[0]), b1=f32(p.conv1[0].bias), g1=f32(p.norm1.gamma), be1=f32(p.norm1.beta), w2=cw(p.conv2[0]),
                           b2=f32(p.conv2[0].bias), g2=f32(p.norm2.gamma), be2=f32(p.norm2.beta), w=f32(p.linear_layer.weight.reshape(-1)),
                           b=f32(p.linear_layer.bias))
        P["pitch"] = (f32(va.pitch_bins), f32(va.pitch_embedding.weight))
        P["energy"] = (f32(va.energy_bins), f32(va.energy_embedding.weight))
        P["mel"] = (bf(self.mel_linear.weight), f32(self.mel_linear.bias))
        P["pos"] = f32(self.position_enc)
        self._prepared = P
        return self

    # ---- device pieces ------------------------------------------------------------------------------------------------------------------
    def _embed(self, lib, ids, table, st):
        B, T = ids.shape
        dev, C, h = ids.device, self.hidden, self.halo
        x = torch.empty((B, T, C), dtype=torch.float32, device=dev)
        img = torch.empty((B, T + 2 * h, C), dtype=torch.bfloat16, device=dev)
        _lib.check(lib.ma_fs2_embed_f32(ids.data_ptr(), B, T, C, table.shape[0], h, table.data_ptr(), self._prepared["pos"].data_ptr(),
                                        x.data_ptr(), img.data_ptr(), st), "fs2_embed")
        self.launches += 1
        return x, img

    def _stack(self, lib, name, x, img, lens, st):
        B, T, C = x.shape
        arr, layers = self._prepared[name]
        stack = getattr(self, name)
        plan = _lib.Fs2Plan(len(layers), stack.n_head, C, self.d_inner, self.kernels[0], self.groups, self.halo, 0, B, T, _NORM_EPS, 0, arr)
        nbytes = int(lib.ma_fs2_workspace_bytes(ctypes.byref(plan)))
        if nbytes < 0:
            _lib.check(nbytes, "fs2 plan")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        _lib.check(lib.ma_fs2_fft_stack(ctypes.byref(plan), x.data_ptr(), img.data_ptr(), lens.data_ptr(), ws.data_ptr(), nbytes, st),
                   "fs2_fft_stack")
        self.launches += len(layers) * (4 + B + (4 if self.groups else 2))

    def _predictor_hidden(self, lib, name, img, B, T, st):
        """conv1 + ReLU, LayerNorm, conv2 + ReLU of a VariancePredictor on the operand image -> (B * T, filter) float32."""
        p, dev, C, F, h = self._prepared[name], img.device, self.hidden, self.filter, self.halo
        rows_u = T + 2 * h
        e = _lib.GemmEpilogue()
        e.alpha, e.act = 1.0, _lib.ACT_RELU
        h1 = torch.empty((B * T, F), dtype=torch.float32, device=dev)
        img1 = torch.empty((B, rows_u, F), dtype=torch.bfloat16, device=dev)
        h2 = torch.empty((B * T, F), dtype=torch.float32, device=dev)
        e.bias = p["b1"].data_ptr()
        for b in range(B):
            _lib.check(lib.ma_conv1d_taps_bf16(img.data_ptr() + (b * rows_u + h) * C * 2, C, T, C, self.vk, 1, p["w1"].data_ptr(),
                                               h1.data_ptr() + b * T * F * 4, F, F, ctypes.byref(e), st), "fs2 predictor conv1")
        _lib.check(lib.ma_fs2_layernorm_pack_f32(h1.data_ptr(), B, T, F, h, p["g1"].data_ptr(), p["be1"].data_ptr(), _LN_EPS, None, None,
                                                 img1.data_ptr(), st), "fs2 predictor norm1")
        e.bias = p["b2"].data_ptr()
        for b in range(B):
            _lib.check(lib.ma_conv1d_taps_bf16(img1.data_ptr() + (b * rows_u + h) * F * 2, F, T, F, self.vk, 1, p["w2"].data_ptr(),
                                               h2.data_ptr() + b * T * F * 4, F, F, ctypes.byref(e), st), "fs2 predictor conv2")
        self.launches += 2 * B + 1
        return h2

    def _head(self, lib, name, h2, B, T, lens, control, st, bins=None, table=None, index_in=None, x=None, pos=None):
        p, dev, C = self._prepared[name], h2.device, self.hidden
        pred = torch.empty((B, T), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        index = x_out = x_pos = img = None
        if table is not None:
            index = torch.empty((B, T), dtype=torch.int32, device=dev)
            x_out = torch.empty((B, T, C), dtype=torch.float32, device=dev)
            x_pos = torch.empty((B, T, C), dtype=torch.float32, device=dev) if pos is not None else None
            img = torch.empty((B, T + 2 * self.halo, C), dtype=torch.bfloat16, device=dev)
        _lib.check(lib.ma_variance_head_f32(h2.data_ptr(), B, T, self.filter, p["g2"].data_ptr(), p["be2"].data_ptr(), _LN_EPS, p["w"].data_ptr(),
                                            p["b"].data_ptr(), ptr(lens), float(control), pred.data_ptr(), ptr(bins), self.n_bins,
                                            ptr(index_in), ptr(index), ptr(table), ptr(x), ptr(pos), C, self.halo, ptr(x_out), ptr(x_pos),
                                            ptr(img), st), "fs2 variance head")
        self.launches += 1
        return pred, index, x_out, x_pos, img

    # ---- the call -----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, speakers, texts, src_lens, max_src_len, positions_encoder=None, positions_decoder=None, mel_lens=None,
              max_mel_len=None, p_targets=None, e_targets=None, d_targets=None, p_control=1.0, e_control=1.0, d_control=1.0,
              _overrides=None):
        """fastspeech2_v190.py:149-205.  texts (B, max_src_len) integer ids padded with 0 = PAD beyond src_lens (B); `speakers` is ignored
        (speaker_emb is None in the reference).  positions_*, mel_lens, max_mel_len and the targets must be None (the reference's infer
        does not use them either, except for tables given in place of the built-in ones).  -> the reference's dict, tensors on the
        device, all rows (padded ones included), plus `pitch_index` / `energy_index` (B, T) int32.
        _overrides: {"durations": (B, T_src) float, "pitch_index": (B, T) int, "energy_index": (B, T) int}, each optional: the discrete
        decisions to use in place of the predicted ones (the predictions are still computed and returned).
        ValueError for a mel longer than max_seq_len + 1 frames or with no frame at all, and for texts whose PAD tokens do not match
        src_lens where that can be seen without a device read-back (texts on the host)."""
        for name, v in (("positions_encoder", positions_encoder), ("positions_decoder", positions_decoder), ("mel_lens", mel_lens),
                        ("max_mel_len", max_mel_len), ("p_targets", p_targets), ("e_targets", e_targets), ("d_targets", d_targets)):
            if v is not None:
                raise NotImplementedError("infer(%s=...) is not built" % name)
        _host.require_gpu()
        dev = self.mel_linear.weight.device
        if dev.type != "cuda":
            raise ValueError("the model's parameters must be on the HIP device (there is no CPU path)")
        ov = dict(_overrides or {})
        texts_t = torch.as_tensor(texts)
        lens_t = torch.as_tensor(src_lens).reshape(-1)
        if texts_t.dim() != 2 or lens_t.numel() != texts_t.shape[0]:
            raise ValueError("texts must be (B, max_src_len) and src_lens (B,)")
        B, Ts = texts_t.shape
        if int(max_src_len) != Ts:
            raise ValueError("max_src_len must equal texts.shape[1]")
        if Ts > self.max_seq_len + 1:
            raise ValueError("texts longer than max_seq_len + 1 have no position encoding")
        if not texts_t.is_cuda and not lens_t.is_cuda:
            pad_pos = texts_t == PAD
            want = torch.arange(Ts)[None, :] >= lens_t.to(torch.int64)[:, None]
            if not torch.equal(pad_pos, want):
                raise ValueError("texts must hold PAD (0) exactly at the positions >= src_lens (the encoder masks by PAD tokens)")
        if self._prepared is None or self._prepared["pos"].device != dev:
            self.prepare()
        P, lib, C, h = self._prepared, _lib.load(), self.hidden, self.halo
        ids = texts_t.to(device=dev, dtype=torch.int32).contiguous()
        lens = lens_t.to(device=dev, dtype=torch.int32).contiguous()
        self.launches = 0
        with _host.pinned_stream():
            st = _host.current_stream_ptr()
            # encoder (models.py:52-74)
            x, img = self._embed(lib, ids, P["encoder.emb"], st)
            self._stack(lib, "encoder", x, img, lens, st)
            # duration predictor, rounding rule, length regulator on the token ids (variance_adapter.py:286-293)
            h2 = self._predictor_hidden(lib, "duration_predictor", img, B, Ts, st)
            logd = self._head(lib, "duration_predictor", h2, B, Ts, lens, 1.0, st)[0]
            dur = torch.empty((B, Ts), dtype=torch.float32, device=dev)
            if "durations" in ov:
                dur.copy_(torch.as_tensor(ov["durations"]).to(device=dev, dtype=torch.float32).reshape(B, Ts))
            else:
                _lib.check(lib.ma_fs2_durations_f32(logd.data_ptr(), B * Ts, float(d_control), dur.data_ptr(), st), "fs2_durations")
                self.launches += 1
            cap = self.max_seq_len + 1
            mel_len = torch.empty((B,), dtype=torch.int32, device=dev)
            expanded = torch.empty((B, cap), dtype=torch.int32, device=dev)
            _lib.check(lib.ma_length_regulate_i32(dur.data_ptr(), ids.data_ptr(), B, Ts, None, mel_len.data_ptr(), expanded.data_ptr(), cap,
                                                  st), "length_regulate")
            self.launches += 1
            T = int(mel_len.max().item())  # the one read-back of an infer: it sizes everything below
            if T > cap:
                raise ValueError("the predicted mel has %d frames, more than max_seq_len + 1 = %d" % (T, cap))
            if T < 1:
                raise ValueError("every predicted duration is 0: there is no frame to decode")
            ids_exp = expanded[:, :T].contiguous()
            # expanded encoder on the expanded ids (fastspeech2_v190.py:192; its masks are ids == PAD)
            x, img = self._embed(lib, ids_exp, P["expanded_encoder.emb"], st)
            self._stack(lib, "expanded_encoder", x, img, mel_len, st)
            # frame-level pitch and energy, mask = None (variance_adapter.py:305-318)
            idx_in = lambda k: torch.as_tensor(ov[k]).to(device=dev, dtype=torch.int32).reshape(B, T).contiguous() if k in ov else None
            h2 = self._predictor_hidden(lib, "pitch_predictor", img, B, T, st)
            pitch, pidx, x, _, img = self._head(lib, "pitch_predictor", h2, B, T, None, p_control, st, bins=P["pitch"][0],
                                                table=P["pitch"][1], index_in=idx_in("pitch_index"), x=x)
            h2 = self._predictor_hidden(lib, "energy_predictor", img, B, T, st)
            energy, eidx, out, x, img = self._head(lib, "energy_predictor", h2, B, T, None, e_control, st, bins=P["energy"][0],
                                                   table=P["energy"][1], index_in=idx_in("energy_index"), x=x, pos=P["pos"])
            # decoder (models.py:112-132) and mel_linear
            self._stack(lib, "decoder", x, img, mel_len, st)
            rows_u = T + 2 * h
            mel_all = torch.empty((B, rows_u, self.n_mels), dtype=torch.float32, device=dev)
            e = _lib.GemmEpilogue()
            e.alpha, e.bias = 1.0, P["mel"][1].data_ptr()
            _lib.check(lib.ma_gemm_bf16(img.data_ptr(), C, P["mel"][0].data_ptr(), C, mel_all.data_ptr(), self.n_mels, B * rows_u, self.n_mels,
                                        C, ctypes.byref(e), st), "fs2 mel_linear")
            self.launches += 1
        ar = torch.arange(T, device=dev)[None, :]
        return {
            "output": out, "pitch_predictions": pitch, "energy_predictions": energy, "log_duration_predictions": logd,
            "duration_rounded": dur, "mel_len": mel_len.to(torch.float32), "mel_masks": (ar >= mel_len[:, None])[:, None, :],
            "mel_predictions": mel_all[:, h:h + T, :], "src_masks": torch.arange(Ts, device=dev)[None, :] >= lens[:, None],
            "src_lens": src_lens, "pitch_index": pidx, "energy_index": eidx,
        }

