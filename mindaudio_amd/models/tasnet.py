"""TasNet on MI355X - mirror of mindaudio.models.tasnet.TasNet (tasnet.py:8-165), forward only (inference and evaluation).

  Encoder    ma_tasnet_gated_encode_f32 (csrc/tasnet.hip): per segment the L2 norm, relu(U x) * sigmoid(V x) -> mixture_w (B, K, N)
             float32, and the separator's LayerNorm (MindSpore's epsilon 1e-7) stored as bf16 straight into the LSTM stack's time-major
             (K, B, Kpad) input.
  Separator  the unidirectional LSTM stack, by one of two schedules:
               "pipelined"  ma_lstm_stack_bf16 (csrc/lstm_stack.hip): one launch per diagonal t + layer, every active layer in it;
               "layered"    ma_lstm_bidir_bf16(dir_mask=1) (csrc/lstm.hip), one call per layer: the cross-check and the yardstick.
             Both round at the same points (x, the weights and every h that feeds a product are bf16).  Then fc as ma_gemm_bf16 with
             the bias in its epilogue -> score (K * B, nspk * N) float32.
  Decoder    ma_tasnet_mask_decode_f32: softmax over the speakers, x mixture_w, basis_signals (weight and bias), x norm_coef (the
             reference multiplies the bias too), stored as (B, nspk, K, L).
PyTorch modules are parameter containers named as the reference's cells (their forward() is never called).  The reference's unused
`separator.new_lstm = Dense(500, 512)` is not a parameter here; utils.ckpt drops it on load and writes it back on save."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _host, _lib
from . import _lstm

__all__ = ["TasNet"]

LN_EPS = 1e-7  # mindspore.nn.LayerNorm's default epsilon
SCHEDULES = ("pipelined", "layered")


class _Encoder(nn.Module):
    def __init__(self, L, N):
        super().__init__()
        self.conv1d_U = nn.Conv1d(L, N, 1)
        self.conv1d_V = nn.Conv1d(L, N, 1)
        for m in (self.conv1d_U, self.conv1d_V):  # weight_init="XavierUniform"
            nn.init.xavier_uniform_(m.weight)


class _LayerNorm(nn.Module):  # MindSpore's parameter names
    def __init__(self, n):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(n))
        self.beta = nn.Parameter(torch.zeros(n))


class _LSTM(nn.Module):  # nn.LSTM(N, hidden, num_layers): the parameter names of a unidirectional stack
    def __init__(self, input_size, hidden, layers):
        super().__init__()
        k = 1.0 / float(np.sqrt(hidden))
        for l in range(layers):
            for name, shape in (("weight_ih", (4 * hidden, input_size if l == 0 else hidden)), ("weight_hh", (4 * hidden, hidden)),
                                ("bias_ih", (4 * hidden,)), ("bias_hh", (4 * hidden,))):
                self.register_parameter("%s_l%d" % (name, l), nn.Parameter(torch.empty(shape).uniform_(-k, k)))


class _Separator(nn.Module):
    def __init__(self, N, hidden, layers, nspk):
        super().__init__()
        self.layer_norm = _LayerNorm(N)
        self.lstm = _LSTM(N, hidden, layers)
        self.fc = nn.Linear(hidden, nspk * N)
        nn.init.xavier_uniform_(self.fc.weight)


class _Decoder(nn.Module):
    def __init__(self, N, L):
        super().__init__()
        self.basis_signals = nn.Linear(N, L)
        nn.init.xavier_uniform_(self.basis_signals.weight)


class TasNet(nn.Module):
    """TasNet(L, N, hidden_size, num_layers, bidirectional=False, nspk=2, schedule="pipelined"): the reference's arguments plus
    `schedule` ("pipelined" | "layered", see the module docstring; it may also be set on the instance between calls).
    Not built (NotImplementedError): bidirectional=True, hidden_size % 64 != 0, L > 64, N > 1024, nspk outside 1 .. 4,
    num_layers outside 1 .. 8.

    model(mixture (B, K, L) NumPy or device tensor) -> est_source (B, nspk, K, L) float32 on the device."""

    def __init__(self, L, N, hidden_size, num_layers, bidirectional=False, nspk=2, schedule="pipelined"):
        super().__init__()
        if bidirectional:
            raise NotImplementedError(
                "bidirectional=True is not built, and the reference cannot run it either: its fc is Dense(hidden_size, nspk * N) "
                "applied to the 2 * hidden_size wide output of a bidirectional nn.LSTM")
        if hidden_size % 64 or hidden_size < 64 or hidden_size > 4096:
            raise NotImplementedError("hidden_size must be a multiple of 64, at most 4096")
        if not 1 <= L <= 64 or not 1 <= N <= 1024:
            raise NotImplementedError("the encoder and decoder kernels are built for L <= 64 and N <= 1024")
        if not 1 <= nspk <= 4 or not 1 <= num_layers <= 8:
            raise NotImplementedError("nspk must be 1 .. 4 and num_layers 1 .. 8")
        if schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s" % (SCHEDULES,))
        self.L, self.N, self.hidden_size, self.num_layers = L, N, hidden_size, num_layers
        self.bidirectional, self.nspk, self.schedule = bidirectional, nspk, schedule
        self.encoder = _Encoder(L, N)
        self.separator = _Separator(N, hidden_size, num_layers, nspk)
        self.decoder = _Decoder(N, L)
        self._prepared = None
        self._ws = {}
        # weights loaded after a forward must be used: any load_state_dict drops the packed copies of prepare()
        self.register_load_state_dict_post_hook(lambda module, _keys: setattr(module, "_prepared", None))

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def load_weights(self, state, strict=True):
        """{reference name: array} -> the module's parameters (the names of utils.ckpt.convert_tasnet_names; Conv1d weights (N, L, 1)
        or MindSpore's (N, L, 1, 1))."""
        from ..utils.ckpt import convert_tasnet_names

        return _lstm.load_named_weights(self, convert_tasnet_names(state), strict, reshape=True)

    def load_checkpoint(self, path, strict=True):
        from ..utils.ckpt import load_mindspore_checkpoint

        return load_mindspore_checkpoint(self, path, strict=strict)

    @torch.no_grad()
    def prepare(self):
        """Device copies in the kernels' layouts: transposed encoder weights, both packings of the LSTM weights, the bf16 fc weight."""
        f32, bf = torch.float32, torch.bfloat16
        H, N = self.hidden_size, self.N
        self._ws = {}
        enc, sep, lstm = self.encoder, self.separator, self.separator.lstm

        def f(t):
            return t.detach().to(f32).contiguous()

        P = {"Ut": f(enc.conv1d_U.weight.squeeze(-1).t()), "bU": f(enc.conv1d_U.bias),  # (L, N)
             "Vt": f(enc.conv1d_V.weight.squeeze(-1).t()), "bV": f(enc.conv1d_V.bias),
             "gamma": f(sep.layer_norm.gamma), "beta": f(sep.layer_norm.beta),
             "fc": sep.fc.weight.detach().to(bf).contiguous(), "fc_bias": f(sep.fc.bias),
             "basis": f(self.decoder.basis_signals.weight), "basis_bias": f(self.decoder.basis_signals.bias),  # (L, N), (L)
             "layers": [], "layered": []}  # one entry per layer and schedule: pipelined, layered
        for k in range(self.num_layers):
            K = N if k == 0 else H
            src = [f(getattr(lstm, "%s_l%d" % (n, k))) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            P["layers"].append(_lstm.pack_stack_layer(src, K, H))
            P["layered"].append(_lstm.pack_bidir_layer(src, None, K, H))
        for what in ("packed", "bias"):  # ma_lstm_stack_bf16 takes one pointer per layer
            P[what + "_ptrs"] = (ctypes.c_void_p * self.num_layers)(*[L[what].data_ptr() for L in P["layers"]])
        self._prepared = P
        return self

    def _workspace(self, B, K, dev):
        key = (B, K, str(dev), int(torch.cuda.current_stream().cuda_stream))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 2:
                self._ws.clear()
            H, N, f32 = self.hidden_size, self.N, torch.float32
            nbytes = _lib.load().ma_lstm_stack_workspace_bytes(K, B, H, self.num_layers)
            if nbytes < 0:
                _lib.check(int(nbytes), "lstm_stack_workspace_bytes")
            ld = (self.nspk * N + 7) // 8 * 8
            ws = self._ws[key] = dict(
                _lstm.layer_buffers(K, B, H, dev), ld=ld,  # (the pipelined schedule writes into the first of its output buffers)
                mw=torch.empty((B, K, N), dtype=f32, device=dev), coef=torch.empty((B, K), dtype=f32, device=dev),
                xin=torch.zeros((K, B, _lstm.ceil64(N)), dtype=torch.bfloat16, device=dev),  # columns past N stay zero
                score=torch.empty((K * B, ld), dtype=f32, device=dev),
                stack=torch.empty((int(nbytes),), dtype=torch.uint8, device=dev))
        return ws

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def _device_input(self, mixture):
        _host.require_gpu()
        dev = self.separator.fc.weight.device
        if dev.type != "cuda":
            raise ValueError("the model's parameters must be on the HIP device (there is no CPU path)")
        if not isinstance(mixture, torch.Tensor):
            mixture = torch.from_numpy(np.ascontiguousarray(np.asarray(mixture, np.float32)))
        if mixture.dim() != 3 or mixture.shape[2] != self.L:
            raise ValueError("mixture must be (B, K, %d)" % self.L)
        if self._prepared is None or self._prepared["fc"].device != dev:
            self.prepare()
        return mixture.to(dev, torch.float32).contiguous(), dev

    @torch.no_grad()
    def encode(self, mixture):
        """(B, K, L) -> (mixture_w (B, K, N) float32, norm_coef (B, K) float32, the stack's input (K, B, Kpad) bf16): views of the
        model's workspace."""
        x, dev = self._device_input(mixture)
        B, K, _ = x.shape
        P, ws = self._prepared, self._workspace(B, K, dev)
        with _host.pinned_stream():
            _lib.check(_lib.load().ma_tasnet_gated_encode_f32(
                x.data_ptr(), B, K, self.L, self.N, P["Ut"].data_ptr(), P["bU"].data_ptr(), P["Vt"].data_ptr(), P["bV"].data_ptr(),
                P["gamma"].data_ptr(), P["beta"].data_ptr(), LN_EPS, ws["mw"].data_ptr(), ws["coef"].data_ptr(), ws["xin"].data_ptr(),
                ws["xin"].shape[2], _host.current_stream_ptr()), "tasnet_gated_encode")
        return ws["mw"], ws["coef"], ws["xin"]

    @torch.no_grad()
    def lstm_stack(self, xin, schedule=None):
        """The separator's LSTM on a (K, B, Kpad) bf16 input: (float32 (K, B, H), its bf16 rounding) of the last layer."""
        schedule = schedule or self.schedule
        if schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s" % (SCHEDULES,))
        P, H = self._prepared, self.hidden_size
        K, B, Kpad = xin.shape
        ws = next(w for w in self._ws.values() if w["xin"] is xin)
        if schedule == "layered":
            return _lstm.run_layers(P["layered"], xin, H, 1, ws)
        of, ob = ws["hf"][0], ws["hb"][0]
        with _host.pinned_stream():
            _lib.check(_lib.load().ma_lstm_stack_bf16(xin.data_ptr(), K, B, Kpad, H, self.num_layers, P["packed_ptrs"], P["bias_ptrs"],
                                                      of.data_ptr(), ob.data_ptr(), None, None, ws["stack"].data_ptr(),
                                                      ws["stack"].numel(), _host.current_stream_ptr()), "lstm_stack")
        return of, ob

    @torch.no_grad()
    def decode(self, hb, mw, coef):
        """fc + softmax + mask + basis_signals on the stack's bf16 output (K, B, H) -> est_source (B, nspk, K, L) float32."""
        P, lib = self._prepared, _lib.load()
        K, B, H = hb.shape
        ws = next(w for w in self._ws.values() if w["mw"] is mw)
        out = torch.empty((B, self.nspk, K, self.L), dtype=torch.float32, device=hb.device)
        e = _lib.GemmEpilogue()
        e.alpha, e.act, e.act2, e.out_bf16, e.bias = 1.0, _lib.ACT_NONE, _lib.ACT_NONE, 0, P["fc_bias"].data_ptr()
        with _host.pinned_stream():
            s = _host.current_stream_ptr()
            _lib.check(lib.ma_gemm_bf16(hb.data_ptr(), H, P["fc"].data_ptr(), H, ws["score"].data_ptr(), ws["ld"], K * B,
                                        self.nspk * self.N, H, ctypes.byref(e), s), "tasnet_fc")
            _lib.check(lib.ma_tasnet_mask_decode_f32(ws["score"].data_ptr(), ws["ld"], mw.data_ptr(), coef.data_ptr(), B, K, self.nspk,
                                                     self.N, P["basis"].data_ptr(), P["basis_bias"].data_ptr(), self.L, out.data_ptr(), s),
                       "tasnet_mask_decode")
        return out

    @torch.no_grad()
    def forward(self, mixture):
        mw, coef, xin = self.encode(mixture)
        _, hb = self.lstm_stack(xin)
        return self.decode(hb, mw, coef)
