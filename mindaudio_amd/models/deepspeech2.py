"""DeepSpeech2 on MI355X - mirror of mindaudio.models.deepspeech2.DeepSpeechModel (deepspeech2.py:190-286), forward only.

  MaskConv   conv1 (1 -> 32, (41, 11), stride (2, 2)) + BN + tanh: ma_ds2_conv1_bf16, a direct float32 kernel that writes the
             (T1 + 10, B, Fpad, 32) bf16 time-major, channel-last activation with its zero frequency rows and halo frames;
             conv2 (32 -> 32, (21, 11), stride (2, 1)) + BN + tanh: one ma_conv1d_taps_bf16 call per output frequency (11 taps over
             time with a dilation of B rows, the 21 frequency taps x 32 channels of that frequency are 704 contiguous columns of a
             row, the 22nd row's weights are zero), BN as the epilogue's column affine, tanh as its second activation; no im2col.
             Nothing is masked, as in the reference: padding frames pass conv, BN and tanh and come out non-zero.
  BatchRNN   ma_lstm_bidir_bf16 per layer (csrc/lstm.hip): both directions over all T1 frames (no lengths), summed.
  fc         ma_gemm_bf16, float32 logits (T1, B, classes).
The features of the LSTM input are ordered f * 32 + c (the layout's order); W_ih of the first layer arrives in the reference's
c * F2 + f order and is permuted in prepare().  BatchNorm is folded on the host: scale = gamma / sqrt(var + 1e-5), shift = beta -
mean * scale.  PyTorch modules are parameter containers named as the reference's cells; their forward() is never called."""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _host, _lib
from . import _lstm

__all__ = ["DeepSpeechModel", "PredictWithSoftmax", "fold_batchnorm", "permute_wih_columns"]

BN_EPS = 1e-5


def fold_batchnorm(gamma, beta, mean, var, eps=BN_EPS):
    """Inference BatchNorm as y = x * scale + shift (float64 arithmetic, float32 result)."""
    g, b, m, v = (np.asarray(a, np.float64) for a in (gamma, beta, mean, var))
    scale = g / np.sqrt(v + eps)
    return scale.astype(np.float32), (b - m * scale).astype(np.float32)


def permute_wih_columns(w_ih, channels, n_freq):
    """(4H, channels * n_freq) with column c * n_freq + f (the reference's reshape of (B, C, F2, T1)) -> column f * channels + c."""
    w = torch.as_tensor(w_ih)
    return w.reshape(w.shape[0], channels, n_freq).permute(0, 2, 1).reshape(w.shape[0], channels * n_freq)


def _conf(audio_conf, key):
    return audio_conf[key] if isinstance(audio_conf, dict) else getattr(audio_conf, key)


class _BatchNorm2d(nn.Module):  # MindSpore's parameter names
    def __init__(self, n):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(n))
        self.beta = nn.Parameter(torch.zeros(n))
        self.moving_mean = nn.Parameter(torch.zeros(n), requires_grad=False)
        self.moving_variance = nn.Parameter(torch.ones(n), requires_grad=False)


class _MaskConv(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, (41, 11), stride=(2, 2), padding=(20, 5), bias=False)
        self.bn1 = _BatchNorm2d(32)
        self.conv2 = nn.Conv2d(32, 32, (21, 11), stride=(2, 1), padding=(10, 5), bias=False)
        self.bn2 = _BatchNorm2d(32)
        for m in (self.conv1, self.conv2):  # deepspeech2.py:101-109
            n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / n))


class _LSTM(nn.Module):  # nn.LSTM(bidirectional=True, has_bias=True): one layer
    def __init__(self, input_size, hidden):
        super().__init__()
        k = 1.0 / math.sqrt(hidden)
        for suffix in ("", "_reverse"):
            for name, shape in (("weight_ih", (4 * hidden, input_size)), ("weight_hh", (4 * hidden, hidden)),
                                ("bias_ih", (4 * hidden,)), ("bias_hh", (4 * hidden,))):
                self.register_parameter(name + "_l0" + suffix, nn.Parameter(torch.empty(shape).uniform_(-k, k)))


class _BatchRNN(nn.Module):
    def __init__(self, input_size, hidden, layers):
        super().__init__()
        self.lstms = nn.ModuleList([_LSTM(input_size if i == 0 else hidden, hidden) for i in range(layers)])


class _SequenceWise(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


class DeepSpeechModel(nn.Module):
    """DeepSpeechModel(batch_size, labels, rnn_hidden_size, nb_layers, audio_conf, rnn_type="LSTM", bidirectional=True): the
    reference's signature.  Not built (NotImplementedError): rnn_type != "LSTM", bidirectional=False, rnn_hidden_size % 64 != 0.

    model(x (B, 1, F, T) float32 device tensor or NumPy, lengths) -> (logits (T1, B, classes) float32, output_lengths)."""

    def __init__(self, batch_size, labels, rnn_hidden_size, nb_layers, audio_conf, rnn_type="LSTM", bidirectional=True):
        super().__init__()
        if rnn_type != "LSTM":
            raise NotImplementedError("rnn_type %r: only LSTM is built (as in the reference)" % (rnn_type,))
        if not bidirectional:
            raise NotImplementedError("only the bidirectional stack is built (as in the reference)")
        if rnn_hidden_size % 64 or rnn_hidden_size < 64:
            raise NotImplementedError("rnn_hidden_size must be a multiple of 64")
        self.batch_size, self.hidden_size, self.hidden_layers = batch_size, rnn_hidden_size, nb_layers
        self.rnn_type, self.audio_conf, self.labels, self.bidirectional = rnn_type, audio_conf, labels, bidirectional
        self.n_freq = int(math.floor(_conf(audio_conf, "sample_rate") * _conf(audio_conf, "window_size") / 2) + 1)
        self.F1 = (self.n_freq - 1) // 2 + 1
        self.F2 = (self.F1 - 1) // 2 + 1
        self.rnn_input_size = 32 * self.F2
        self.conv = _MaskConv()
        self.pre, self.stride = self.get_conv_num()
        self.RNN = _BatchRNN(self.rnn_input_size, rnn_hidden_size, nb_layers)
        fc = nn.Linear(rnn_hidden_size, len(labels), bias=False)
        nn.init.uniform_(fc.weight, -1.0 / rnn_hidden_size, 1.0 / rnn_hidden_size)  # deepspeech2.py:36-45
        self.fc = _SequenceWise(fc)
        self._prepared = None
        self._ws = {}
        # weights loaded after a forward must be used: any load_state_dict drops the packed copies of prepare()
        self.register_load_state_dict_post_hook(lambda module, _keys: setattr(module, "_prepared", None))

    # ---- lengths ---------------------------------------------------------------------------------------------------------------
    def get_conv_num(self):
        p, s = [], []
        for conv in (self.conv.conv1, self.conv.conv2):  # deepspeech2.py:277-286 on the time axis
            k = conv.kernel_size[1]
            p.append(2 * int((k - 1) / 2) - conv.dilation[1] * (k - 1) - 1)
            s.append(conv.stride[1])
        return p, s

    def get_seq_lens(self, seq_len):
        """deepspeech2.py:266-275 on int32 lengths: len = (len + pre) / stride + 1 per convolution, the division truncating like the
        reference's int32 Div (for len >= 1 the numerator is >= 0, where truncation and floor agree)."""
        v = np.asarray(seq_len.detach().cpu() if hasattr(seq_len, "detach") else seq_len).astype(np.int32)
        for pre, stride in zip(self.pre, self.stride):
            num = v + np.int32(pre)
            v = (np.sign(num) * (np.abs(num) // stride)).astype(np.int32) + np.int32(1)
        return v

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def load_weights(self, params, strict=True):
        """{reference name: array} -> the module's parameters (the names of utils.ckpt.convert_deepspeech2_names)."""
        return _lstm.load_named_weights(self, params, strict)

    def load_checkpoint(self, path, strict=True):
        from ..utils.ckpt import load_mindspore_checkpoint

        return load_mindspore_checkpoint(self, path, strict=strict)

    @torch.no_grad()
    def prepare(self):
        f32, bf = torch.float32, torch.bfloat16
        self._ws = {}
        P = {"layers": []}
        self._fold_frontend(P)
        for k, cell in enumerate(self.RNN.lstms):
            fwd, bwd = ([getattr(cell, n + "_l0" + d).detach().to(f32) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                        for d in ("", "_reverse"))
            if k == 0:
                fwd[0], bwd[0] = permute_wih_columns(fwd[0], 32, self.F2), permute_wih_columns(bwd[0], 32, self.F2)
            P["layers"].append(_lstm.pack_bidir_layer(fwd, bwd, self.rnn_input_size if k == 0 else self.hidden_size, self.hidden_size))
        P["fc"] = self.fc.module.weight.detach().to(bf).contiguous()
        self._prepared = P
        return self

    @torch.no_grad()
    def _fold_frontend(self, P):
        """MaskConv's inference operands into P: conv1 tap-major, both BatchNorms folded, conv2 as 11 taps over time.  A trainer that has
        changed the convolutions or the moving statistics sets P["frontend_stale"]; frontend() then comes back here."""
        dev = self.fc.module.weight.device
        f32, bf = torch.float32, torch.bfloat16
        c = self.conv
        P.pop("frontend_stale", None)
        P["w1t"] = c.conv1.weight.detach().to(f32).reshape(32, 41 * 11).t().contiguous()  # (451, 32)
        for i, bn in ((1, c.bn1), (2, c.bn2)):
            sc, sh = fold_batchnorm(*(p.detach().cpu().numpy() for p in (bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance)))
            P["scale%d" % i], P["shift%d" % i] = torch.from_numpy(sc).to(dev), torch.from_numpy(sh).to(dev)
        # conv2 as 11 taps over time x (22 frequency rows x 32 channels): W[n, j, df * 32 + c] = w2[n, c, df, j], row 21 zero
        w2 = torch.zeros((32, 11, 22, 32), dtype=f32, device=dev)
        w2[:, :, :21, :] = c.conv2.weight.detach().to(f32).permute(0, 3, 2, 1)
        P["w2"] = w2.reshape(32, 11 * 704).to(bf).contiguous()

    def _workspace(self, B, F, T, dev):
        key = (B, F, T, str(dev), int(torch.cuda.current_stream().cuda_stream))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 2:
                self._ws.clear()
            bf = torch.bfloat16
            T1 = (T - 1) // 2 + 1
            Fpad = 2 * (self.F2 - 1) + 22
            ws = self._ws[key] = dict(
                _lstm.layer_buffers(T1, B, self.hidden_size, dev), T1=T1, Fpad=Fpad,
                act1=torch.zeros((T1 + 10, B, Fpad * 32), dtype=bf, device=dev),  # halo frames and padding rows stay zero
                xin=torch.zeros((T1, B, _lstm.ceil64(self.rnn_input_size)), dtype=bf, device=dev))  # columns past 32 F2 stay zero
        return ws

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def frontend(self, x):
        """MaskConv on x (B, 1, F, T): the (T1, B, Kpad) bf16 LSTM input, feature f * 32 + c (a view of the model's workspace)."""
        _host.require_gpu()
        dev = self.fc.module.weight.device
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.n_freq:
            raise ValueError("x must be (B, 1, %d, T)" % self.n_freq)
        if not dev.type == "cuda":
            raise ValueError("the model's parameters must be on the HIP device (there is no CPU path)")
        x = x.to(dev, torch.float32).contiguous()
        if self._prepared is None or self._prepared["fc"].device != dev:
            self.prepare()
        P, lib, ck = self._prepared, _lib.load(), _lib.check
        if P.get("frontend_stale"):
            self._fold_frontend(P)
        B, _, F, T = x.shape
        ws = self._workspace(B, F, T, dev)
        T1, Fpad, act1, xin = ws["T1"], ws["Fpad"], ws["act1"], ws["xin"]
        lda, Kpad = Fpad * 32, xin.shape[2]
        e = _lib.GemmEpilogue()
        e.alpha, e.act, e.act2, e.out_bf16 = 1.0, _lib.ACT_NONE, _lib.ACT_TANH, 1
        e.col_scale, e.col_shift = P["scale2"].data_ptr(), P["shift2"].data_ptr()
        with _host.pinned_stream():
            s = _host.current_stream_ptr()
            ck(lib.ma_ds2_conv1_bf16(x.data_ptr(), B, F, T, P["w1t"].data_ptr(), P["scale1"].data_ptr(), P["shift1"].data_ptr(), Fpad,
                                     act1.data_ptr(), s), "ds2_conv1")
            first = act1.data_ptr() + 5 * B * lda * 2  # frame 0 of the interior: the taps reach 5 frames = 5 B rows to either side
            for fo in range(self.F2):
                ck(lib.ma_conv1d_taps_bf16(first + 2 * fo * 32 * 2, lda, T1 * B, 704, 11, B, P["w2"].data_ptr(),
                                           xin.data_ptr() + fo * 32 * 2, Kpad, 32, ctypes.byref(e), s), "ds2_conv2")
        return xin

    @torch.no_grad()
    def lstm_stack(self, xin):
        """The BatchRNN on a (T1, B, Kpad) bf16 input: (float32 (T1, B, H), its bf16 rounding) of the last layer."""
        ws = next(w for w in self._ws.values() if w["xin"] is xin)
        return _lstm.run_layers(self._prepared["layers"], xin, self.hidden_size, 3, ws)

    @torch.no_grad()
    def forward(self, x, lengths):
        output_lengths = self.get_seq_lens(lengths)
        xin = self.frontend(x)
        _, hb = self.lstm_stack(xin)
        T1, B, H = hb.shape
        C = len(self.labels)
        ldc = (C + 7) // 8 * 8
        logits = torch.empty((T1, B, ldc), dtype=torch.float32, device=hb.device)
        e = _lib.GemmEpilogue()
        e.alpha, e.act, e.act2, e.out_bf16 = 1.0, _lib.ACT_NONE, _lib.ACT_NONE, 0
        _lib.check(_lib.load().ma_gemm_bf16(hb.data_ptr(), H, self._prepared["fc"].data_ptr(), H, logits.data_ptr(), ldc, T1 * B, C, H,
                                            ctypes.byref(e), _host.current_stream_ptr()), "ds2_fc")
        return logits[:, :, :C], output_lengths

    @torch.no_grad()
    def predict(self, x, lengths):
        """PredictWithSoftmax (examples/deepspeech2/eval.py:17-33): (probabilities (B, T1, classes), output_lengths)."""
        logits, out_len = self.forward(x, lengths)
        T1, B, C = logits.shape
        probs = torch.empty((B, T1, C), dtype=torch.float32, device=logits.device)
        _lib.check(_lib.load().ma_ds2_softmax_f32(logits.data_ptr(), logits.stride(1), T1, B, C, probs.data_ptr(),
                                                  _host.current_stream_ptr()), "ds2_softmax")
        return probs, out_len


class PredictWithSoftmax:
    """eval.py's wrapper: model(inputs, input_length) -> (softmax probabilities (B, T1, classes), output sizes); the lengths are cast
    to int32 as the reference casts them."""

    def __init__(self, network):
        self.network = network

    def __call__(self, inputs, input_length):
        n = input_length.detach().cpu().numpy() if hasattr(input_length, "detach") else np.asarray(input_length)
        return self.network.predict(inputs, n.astype(np.int32))
