"""WaveGrad training step on MI355X: the model's own forward with every buffer kept, the L1 loss, a hand-written backward and
MyTrainOneStepCell's unscale / clip_by_global_norm / nn.Adam (examples/wavegrad/train.py:25-62, 150-170 around
mindaudio/models/wavegrad/wavegrad_v190.py).

The forward IS WaveGrad's: the trainer takes the model's op list (WaveGrad._build_ops), gives every buffer a block of its own and, in
bf16 mode, calls ma_wavegrad_forward on it, so `pred` has the bits of WaveGrad.forward.  The backward is that list walked in reverse, a
Python loop of C calls.  Per op:
  LAST  ma_wavegrad_l1_last_bwd_f32: loss, g = d loss / d pred, the gradient of last_conv's input, partials of its dw / db;
  CONV  the gradient of the output becomes an operand image through the forward's producer (slope 1, mul = alpha); dX is
        ma_conv1d_taps_bf16 on the transposed, tap-reversed weight copy (one call per utterance, further consumers of the same operand
        added through the residual epilogue); dW is ma_gemm_tn_bf16_f32 once per tap over the whole batch, straight into the
        (N, taps, C) gradient, db the colsum of the centre tap; the residual's gradient is the output's (the same buffer);
  DOWN  dX ma_gemm_bf16 against the transposed weight, dW the TN product per utterance, accumulated in utterance order;
  PACK  ma_wavegrad_pack_bwd_f32 (LeakyReLU mask from the recomputed forward value, FiLM shift / scale gradients, repetition sum);
  INIT  ma_wavegrad_init_conv_bwd_f32 (partials).
One ma_reduce_splits_batch_f32 launch sums the partials of last_conv and the init convolution.  `operands="f32"` is the validation mode:
the same walk with float32 operand images (ma_wavegrad_pack_f32) and every product through ma_gemm_x32 / ma_colsum_x32, one call per
tap and utterance.

The parameters, the gradient and both Adam moments are a train.flat.FlatParams (8-element alignment), so the norm and the update are
one launch each.  Convolution weights are kept in the operand order (N, taps, C) and the model's parameters become permuted views of
them ((out, in, k) as the reference names them); the init convolution is kept (taps, C0), the order its forward kernel reads.  The bf16 operand copies (padded, and the transposed ones of the input gradients) are rewritten by one
ma_wavegrad_weights_bf16 launch after an update.  Moving the model to another device after the trainer has bound it is not supported."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _host, _lib
from ..train import plans
from ..train.flat import (ADAM_BETA1, ADAM_BETA2, DynamicLossScale, FlatTrainer, adam_lr_t, stored_last_first,
                          stored_taps_inner)
from .wavegrad import WaveGrad, _pad64, positional_table

__all__ = ["WaveGradTrainer"]

_EPS = 1e-8  # nn.Adam's default (train.py:130 passes only the learning rate)
_F32, _BF16 = torch.float32, torch.bfloat16


def _epilogue(alpha=1.0, bias=None, residual=None, ldr=0):
    e = _lib.GemmEpilogue()
    e.alpha, e.act, e.act2, e.out_bf16 = alpha, _lib.ACT_NONE, _lib.ACT_NONE, 0
    if bias is not None:
        e.bias = bias
    if residual is not None:
        e.residual, e.ldr = residual, ldr
    return e


# ---- the products of the backward pass (every pointer is a device address; -> kernel launches) ------------------------------------------
def conv_dw(lib, bf, gimg, np_, ximg, cp, gw, gb, n, c, taps, d, rows_all, tn_ws, tn_bytes, s):
    """dW of a `taps`-tap "same" convolution, one product per tap over the WHOLE batch: gimg (rows_all, np_) is the operand image of the
    output gradient and ximg (rows_all, cp) the saved forward operand, both with >= (taps / 2) * d zero halo rows around every utterance
    in gimg, which cut the utterances apart.  gw (n, taps, c) float32 is stored, gb (n) added to (bf16) / stored (f32)."""
    ck, esz, half, count = _lib.check, 2 if bf else 4, taps // 2, 0
    for j in range(taps):
        sh = (j - half) * d
        a, x = gimg + max(0, -sh) * np_ * esz, ximg + max(0, sh) * cp * esz
        if bf:
            ck(lib.ma_gemm_tn_bf16_f32(a, np_, x, cp, gw + j * c * 4, taps * c, n, c, rows_all - abs(sh), n, 1.0, 0, gb if j == half else None,
                                       tn_ws, tn_bytes, s), "dW")
            count += 3 if j == half else 2
        else:
            ck(lib.ma_gemm_x32(a, 1, np_, x, 1, cp, gw + j * c * 4, taps * c, n, c, rows_all - abs(sh), None, s), "gemm_x32 dW")
            count += 1
    if not bf:
        ck(lib.ma_colsum_x32(gimg, np_, rows_all, n, gb, 0, s), "colsum_x32")
        count += 1
    return count


def conv_dx(lib, bf, gimg, np_, w, out, ld, acc, B, T, h, n, c, taps, d, s):
    """dX of the same convolution into out (B, T, ld >= c) float32, one call per utterance (and per tap in float32 mode); acc: added to
    what is there, through the residual epilogue.  w: bf16 (c, taps, np_) tap-reversed, or the float32 master (n, taps, c)."""
    ck, rows_u, half = _lib.check, T + 2 * h, taps // 2
    for b in range(B):
        o = out + b * T * ld * 4
        if bf:
            e = _epilogue(1.0, None, o if acc else None, ld)
            ck(lib.ma_conv1d_taps_bf16(gimg + ((b * rows_u + h) * np_) * 2, np_, T, np_, taps, d, w, o, ld, c, ctypes.byref(e), s), "dX")
        else:
            for j in range(taps):
                a = gimg + ((b * rows_u + h - (j - half) * d) * np_) * 4
                e = _epilogue(1.0, None, o if (acc or j > 0) else None, ld)
                ck(lib.ma_gemm_x32(a, np_, 1, w + j * c * 4, 1, taps * c, o, ld, T, c, n, ctypes.byref(e), s), "gemm_x32 dX")
    return B if bf else B * taps


def down_bwd(lib, bf, gimg, np_, ximg, cp, h, w, out, acc, gw, gb, B, T, n, c, f, tn_ws, tn_bytes, s):
    """Backward of the kernel = stride = f convolution: gimg (B, T, np_) the output gradient's image (no halo), ximg (B, T f + 2 h, cp)
    the saved operand.  dX -> out (B, T f, cp) float32 (ma_gemm_bf16 against w (f cp, np_) bf16, or the float32 master (n, f, c)); dW
    (n, f, c) and db are ADDED to gw / gb per utterance, in utterance order."""
    ck, esz, rows_in, count = _lib.check, 2 if bf else 4, T * f + 2 * h, 0
    for b in range(B):
        a = gimg + b * T * np_ * esz
        x = ximg + ((b * rows_in + h) * cp) * esz
        o = out + b * T * f * cp * 4
        e = _epilogue(1.0, None, o if acc else None, f * cp)
        if bf:
            ck(lib.ma_gemm_bf16(a, np_, w, np_, o, f * cp, T, f * cp, np_, ctypes.byref(e), s), "down dX")
            if c == cp:
                ck(lib.ma_gemm_tn_bf16_f32(a, np_, x, f * cp, gw, f * c, n, f * c, T, n, 1.0, 1, gb, tn_ws, tn_bytes, s), "down dW")
                count += 4
            else:  # padded columns: one product per kernel position, so that only the c real columns are read
                for q in range(f):
                    ck(lib.ma_gemm_tn_bf16_f32(a, np_, x + q * cp * 2, f * cp, gw + q * c * 4, f * c, n, c, T, n, 1.0, 1, gb if q == 0 else None,
                                               tn_ws, tn_bytes, s), "down dW")
                count += 2 + 2 * f
        else:
            ck(lib.ma_gemm_x32(a, np_, 1, w, 1, f * c, o, f * c, T, f * c, n, ctypes.byref(e), s), "gemm_x32 down dX")
            ew = _epilogue(1.0, None, gw, f * c)
            ck(lib.ma_gemm_x32(a, 1, np_, x, 1, f * c, gw, f * c, n, f * c, T, ctypes.byref(ew), s), "gemm_x32 down dW")
            count += 2
    if not bf:
        ck(lib.ma_colsum_x32(gimg, np_, B * T, n, gb, 1, s), "colsum_x32")
        count += 1
    return count


class _Step:
    """Everything of one (B, frames) shape: the op list, the activation and gradient arenas, the item table of the partial sums."""


class WaveGradTrainer(FlatTrainer):
    """WaveGradTrainer(model, learning_rate, max_grad_norm=1.0, loss_scale=2**12, scale_factor=2, scale_window=1000, operands="bf16").

    loss_and_grads(noisy_audio (B, T), noise_scale (B,) or (1,), noise (B, T), spectrogram (B, n_mels, T / hop)) -> loss (float), the
        mean |pred - noise|; gradients() then holds d(loss_scale * loss) / d parameter under the names of model.state_dict(), shaped
        (out, in, k); activation_gradients()["pred"] the same for the network's output.
    step(noisy_audio, noise_scale, noise, spectrogram, lr=None) -> (loss, overflow, loss_scale): the same, then the gradient is
        unscaled, clipped by its global norm to max_grad_norm and applied by nn.Adam; a non-finite norm skips the update and halves
        the loss scale (train.flat.DynamicLossScale).  `lr` defaults to learning_rate.
    state_dict() / load_state_dict(): the model's entries plus "moment1.<name>", "moment2.<name>", "steps" and "loss_scale".

    ValueError before any device call for CPU tensors, wrong ranks, T != hop * frames or a `noise` of another shape."""

    def __init__(self, model, learning_rate, max_grad_norm=1.0, loss_scale=2 ** 12, scale_factor=2, scale_window=1000, operands="bf16"):
        if not isinstance(model, WaveGrad):
            raise TypeError("model must be a models.WaveGrad")
        if operands not in ("bf16", "f32"):
            raise ValueError("operands must be 'bf16' or 'f32'")
        if not learning_rate > 0 or not max_grad_norm > 0 or not loss_scale >= 1:
            raise ValueError("learning_rate and max_grad_norm must be positive, loss_scale at least 1")
        self.model, self.learning_rate, self.max_grad_norm = model, float(learning_rate), float(max_grad_norm)
        self.scaler = DynamicLossScale(float(loss_scale), float(scale_factor), int(scale_window))
        self.operands, self.bf16 = operands, operands == "bf16"
        self.steps = 0
        self.last_norm = None
        self.launches = {}
        self._steps = {}
        self._stale = True
        self._act_grads = {}
        model.register_load_state_dict_post_hook(lambda module, _keys: setattr(self, "_stale", True))

    # ---- parameters ---------------------------------------------------------------------------------------------------------------
    def _convs(self):
        """[(module name, Conv1d)] in state_dict order."""
        return [(name, m) for name, m in self.model.named_modules() if isinstance(m, nn.Conv1d)]

    def _bind(self, dev):
        m = self.model
        init, last = m.DBlock[0], m.last_conv
        padded_bias = {id(blk.residual_dense) for blk in list(m.DBlock)[1:]}  # its bf16 output is an operand: 64-column rows
        entries = []
        for name, conv in self._convs():
            w, b = conv.weight, conv.bias
            entries.append((name + ".weight", tuple(w.shape), stored_last_first if conv is init else stored_taps_inner))
            entries.append((name + ".bias", tuple(b.shape), None, _pad64(b.numel()) if id(conv) in padded_bias else b.numel()))
        self._bind_params(entries, dev, mirror_bf16=False, moments=("moment1", "moment2"))
        fp = self.params
        self._norm_parts = int(_lib.load().ma_wavegrad_sumsq_parts(fp.size))
        self._norm_part = torch.zeros(self._norm_parts, dtype=torch.float64, device=dev)
        self._flag = torch.zeros(4, dtype=torch.int32, device=dev)
        self._norm = torch.zeros(4, dtype=_F32, device=dev)
        # what the plan's ops point to: per convolution (forward operand, bias, transposed operand), keyed as WaveGrad.prepare() keys it
        self._P, self._rev, self._by_ptr, items, mo = {}, {}, {}, [], 0
        mfma = [(name, conv) for name, conv in self._convs() if conv is not init and conv is not last]
        downs = {id(c) for blk in list(m.DBlock)[1:] for c in (blk.downscale1, blk.downscale2)}
        if self.bf16:
            sizes = []
            for name, conv in mfma:
                n, c, k = conv.weight.shape
                rows = _pad64(n) if id(conv) in padded_bias else n
                sizes.append((rows * k * _pad64(c), k * _pad64(c) * _pad64(n) if id(conv) in downs else c * k * _pad64(n)))
            self._mirror = torch.zeros(sum(a + b for a, b in sizes), dtype=_BF16, device=dev)
        for i, (name, conv) in enumerate(mfma):
            n, c, k = conv.weight.shape
            woff, boff = fp.index[name + ".weight"][0], fp.index[name + ".bias"][0]
            rows = _pad64(n) if (self.bf16 and id(conv) in padded_bias) else n
            bias = fp.master[boff:boff + rows]
            if self.bf16:
                fsz, rsz = sizes[i]
                fwd = self._mirror[mo:mo + fsz].view(rows, k, _pad64(c))
                rev = self._mirror[mo + fsz:mo + fsz + rsz]
                mo += fsz + rsz
                mode = 1 if id(conv) in downs else 0
                item = _lib.WaveGradWeightItem(fp.ptr(name + ".weight"), fwd.data_ptr(), rev.data_ptr(), n, k, c, _pad64(c), _pad64(n),
                                               rows, mode, 0)
                items.append((item, (_pad64(n) * k * _pad64(c) + 255) // 256))
                self._rev[name] = rev
            else:
                fwd = fp.master[woff:woff + n * k * c].view(n, k, c)
            self._P[id(conv)] = (fwd, bias)
            self._by_ptr[fwd.data_ptr()] = (name, n, c, k)
        for key, conv in (("init", init), ("last", last)):
            name = [nm for nm, cv in self._convs() if cv is conv][0]
            woff, boff = fp.index[name + ".weight"][0], fp.index[name + ".bias"][0]
            n, c, k = conv.weight.shape
            w = fp.master[woff:woff + n * c * k].view(k, max(n, c))  # (taps, C0) and (taps, C)
            self._P[key] = (w, fp.master[boff:boff + n])
            self._by_ptr[w.data_ptr()] = (name, n, c, k)
        self._weights_plan = plans.ItemTable(items, dev) if self.bf16 else None
        m._drop()
        self._stale = True

    def _refresh(self, s):
        """The bf16 operand copies from the float32 masters: one launch."""
        if self.bf16:
            _lib.check(_lib.load().ma_wavegrad_weights_bf16(*self._weights_plan.args, s), "wavegrad_weights")
        self._stale = False

    def activation_gradients(self):
        return dict(self._act_grads)

    def _extra_state(self):
        return {"loss_scale": torch.tensor(self.scaler.scale, dtype=torch.float64)}

    def _loaded(self, state):
        if "loss_scale" in state:
            self.scaler.scale = float(state["loss_scale"])

    # ---- the plan -----------------------------------------------------------------------------------------------------------------
    def _plan(self, B, frames, dev):
        key = (B, frames)
        st = self._steps.get(key)
        if st is not None:
            return st
        if len(self._steps) >= 2:
            self._steps.clear()
        m, lib, bf = self.model, _lib.load(), self.bf16
        saved, m._prepared = m._prepared, self._P
        try:
            ops, _sizes = m._build_ops(B, frames)
        finally:
            m._prepared = saved
        T = m.hop * frames
        esz = 2 if bf else 4

        def width(c):  # columns of an operand image
            return _pad64(c) if bf else c

        # every buffer of the forward: (bytes, rows per utterance, row length in floats) under its own name, nothing reused
        fsize, rowlen, images = {}, {}, {}
        for op in ops:
            k = op["kind"]
            if k == _lib.WAVEGRAD_OP_INIT:
                fsize[op["out"]], rowlen[op["out"]] = B * op["T"] * op["N"] * 4, (op["T"], op["N"])
            elif k == _lib.WAVEGRAD_OP_PACK:
                if op["out"] is not None:
                    fsize[op["out"]] = B * (op["T"] + 2 * op["halo"]) * width(op["C"]) * esz
                    images[op["out"]] = op
                    rowlen[op["out"]] = (op["T"], width(op["C"]))
                if op["out2"] is not None:
                    fsize[op["out2"]], rowlen[op["out2"]] = B * op["T"] * op["C"] * 4, (op["T"], op["C"])
            elif k in (_lib.WAVEGRAD_OP_CONV, _lib.WAVEGRAD_OP_DOWN):
                fsize[op["out"]] = B * op["T"] * op["N"] * (esz if op.get("out_bf16") else 4)
                rowlen[op["out"]] = (op["T"], op["N"])
        foff, top = {}, 0
        for name, nbytes in fsize.items():
            foff[name] = top
            top += (nbytes + 255) // 256 * 256
        # gradients: one float32 buffer per float32 activation and per operand image (without halo rows); a residual's gradient IS
        # its convolution's output gradient (every residual has one reader)
        alias = {op["residual"]: op["out"] for op in ops if op.get("residual") is not None}
        goff, gtop = {}, 0
        for name, (t, ld) in rowlen.items():
            if name in alias:
                continue
            goff[name] = gtop
            gtop += (B * t * ld * 4 + 255) // 256 * 256
        for name, root in alias.items():
            goff[name] = goff[root]
        prods = [op for op in ops if op["kind"] in (_lib.WAVEGRAD_OP_CONV, _lib.WAVEGRAD_OP_DOWN)]
        gimg_bytes = max(B * (op["T"] + 2 * op["halo"]) * width(op["N"]) * esz for op in prods)
        st = _Step()
        st.ops, st.B, st.T, st.frames, st.foff, st.goff, st.rowlen, st.images = ops, B, T, frames, foff, goff, rowlen, images
        st.ws = torch.zeros(top, dtype=torch.uint8, device=dev)
        st.gws = torch.zeros(gtop, dtype=torch.uint8, device=dev)
        st.gimg = torch.zeros(gimg_bytes + 256, dtype=torch.uint8, device=dev)
        st.pred = torch.empty((B, T), dtype=_F32, device=dev)
        st.g = torch.empty((B, T), dtype=_F32, device=dev)
        st.loss = torch.zeros(2, dtype=torch.float64, device=dev)
        if bf:
            arr = (_lib.WaveGradOp * len(ops))()
            for o, d in zip(arr, ops):
                o.kind, o.once = d["kind"], 0
                o.inp, o.in2, o.out, o.out2, o.residual = (
                    (_lib.WAVEGRAD_BUF_NONE if d.get(r) is None else foff[d[r]] if isinstance(d[r], str) else d[r])
                    for r in ("inp", "in2", "out", "out2", "residual"))
                o.w = d["w"].data_ptr() if d.get("w") is not None else None
                o.bias = d["bias"].data_ptr() if d.get("bias") is not None else None
                o.T, o.ld_film = d["T"], d.get("ld_film", 0)
                o.C, o.Cpad, o.N, o.taps, o.dilation = d.get("C", 0), d.get("Cpad", 0), d.get("N", 0), d.get("taps", 1), d.get("dilation", 1)
                o.f, o.halo, o.out_bf16, o.enc_off = d.get("f", 1), d.get("halo", 0), d.get("out_bf16", 0), d.get("enc_off", -1)
                o.slope, o.mul, o.res_mul, o.alpha = d.get("slope", 1.0), d.get("mul", 1.0), d.get("res_mul", 0.0), d.get("alpha", 1.0)
            st.arr = arr
            st.c = _lib.WaveGradPlan(len(ops), sum(m.enc_dims), B, T, frames, m.n_mels, arr)
            need = int(lib.ma_wavegrad_workspace_bytes(ctypes.byref(st.c)))
            if need < 0:
                _lib.check(need, "wavegrad training plan")
            assert need <= top
            tn = 0
            for op in prods:
                _name, n, c, k = self._by_ptr[op["w"].data_ptr()]
                if op["kind"] == _lib.WAVEGRAD_OP_CONV:
                    tn = max(tn, int(lib.ma_gemm_tn_workspace_bytes(n, c, B * (op["T"] + 2 * op["halo"]))))
                else:
                    tn = max(tn, int(lib.ma_gemm_tn_workspace_bytes(n, k * c if c == _pad64(c) else c, op["T"])))
            st.tn_ws, st.tn_bytes = torch.zeros(tn + 256, dtype=torch.uint8, device=dev), tn
        # partials of last_conv and of the init convolution, and the one launch that sums them
        last, init = ops[-1], ops[0]
        lp, ip = int(lib.ma_wavegrad_last_bwd_parts(B, T)), int(lib.ma_wavegrad_init_bwd_parts(B, T))
        st.last_stride = (last["taps"] * last["C"] + 1 + 7) // 8 * 8
        st.last_part = torch.zeros(lp * st.last_stride, dtype=_F32, device=dev)
        st.loss_part = torch.zeros(lp, dtype=torch.float64, device=dev)
        istride = (init["taps"] + 1) * init["N"]
        st.init_part = torch.zeros(ip * istride, dtype=_F32, device=dev)
        items, fp = [], self.params
        for part, stride, splits, op, nw, nb in ((st.last_part, st.last_stride, lp, last, last["taps"] * last["C"], 1),
                                                 (st.init_part, istride, ip, init, init["taps"] * init["N"], init["N"])):
            name = self._by_ptr[op["w"].data_ptr()][0]
            woff, boff = fp.index[name + ".weight"][0], fp.index[name + ".bias"][0]
            items.append(plans._reduce_item(part.data_ptr(), fp.grad[woff:woff + nw], nw, nw, nw, splits, stride, splits >= 64,
                                            accumulate=False))
            items.append(plans._reduce_item(part.data_ptr() + nw * 4, fp.grad[boff:boff + nb], nb, nb, nb, splits, stride, splits >= 64,
                                            accumulate=False))
        st.reduce = plans.ItemTable(items, dev)
        self._steps[key] = st
        return st

    # ---- calls ----------------------------------------------------------------------------------------------------------------------
    def _check_inputs(self, noisy_audio, noise_scale, noise, spectrogram):
        B, T, frames = self.model._check_inputs(noisy_audio, spectrogram)
        if not torch.is_tensor(noise) or tuple(noise.shape) != (B, T):
            raise ValueError("noise must be a (B, T) tensor of the audio's shape")
        if not noise.is_cuda or noise.device != noisy_audio.device:
            raise ValueError("noise must be on the audio's HIP device (there is no CPU path)")
        levels = np.asarray(noise_scale.detach().cpu() if torch.is_tensor(noise_scale) else noise_scale, np.float64).reshape(-1)
        if levels.size not in (1, B):
            raise ValueError("noise_scale must hold one value, or one per utterance")
        return B, T, frames, levels

    def _count(self, phase, n=1):
        self.launches[phase] = self.launches.get(phase, 0) + n

    def loss_and_grads(self, noisy_audio, noise_scale, noise, spectrogram):
        st = self._run(noisy_audio, noise_scale, noise, spectrogram)
        return float(st.loss[0].item())

    def _run(self, noisy_audio, noise_scale, noise, spectrogram):
        B, T, frames, levels = self._check_inputs(noisy_audio, noise_scale, noise, spectrogram)
        _host.require_gpu()
        dev = noisy_audio.device
        with torch.no_grad():
            if self.params is None:
                self.model.to(dev)
                self._bind(dev)
            elif self.params.master.device != dev:
                raise ValueError("the trainer is bound to %s" % self.params.master.device)
            st = self._plan(B, frames, dev)
            st.enc = torch.from_numpy(positional_table(levels, self.model.enc_dims)).to(dev)
            st.ld_enc = st.enc.shape[1] if levels.size > 1 else 0
            st.audio = noisy_audio.to(_F32).contiguous()
            st.noise = noise.to(_F32).contiguous()
            st.mel = self.model.mel_rows(spectrogram)
            self.launches = {}
            with _host.pinned_stream():
                s = _host.current_stream_ptr()
                if self._stale:
                    self._refresh(s)
                self._forward(st, s)
                self.params.grad.zero_()  # (the bias gradients are column sums that add to what is there)
                self._count("backward")
                self._backward(st, s)
        return st

    def step(self, noisy_audio, noise_scale, noise, spectrogram, lr=None):
        st = self._run(noisy_audio, noise_scale, noise, spectrogram)
        lib, scale, fp = _lib.load(), self.scaler.scale, self.params
        lr = self.learning_rate if lr is None else float(lr)
        lr_t = adam_lr_t(lr, self.steps + 1, ADAM_BETA1, ADAM_BETA2)
        with torch.no_grad(), _host.pinned_stream():
            s = _host.current_stream_ptr()
            _lib.check(lib.ma_wavegrad_sumsq_f64(fp.grad.data_ptr(), fp.size, self._norm_part.data_ptr(), s), "wavegrad_sumsq")
            _lib.check(lib.ma_wavegrad_clip_adam_f32(fp.master.data_ptr(), fp.grad.data_ptr(), fp.moment1.data_ptr(), fp.moment2.data_ptr(),
                                                     fp.size, self._norm_part.data_ptr(), self._norm_parts, scale, self.max_grad_norm,
                                                     lr_t, ADAM_BETA1, ADAM_BETA2, _EPS, self._flag.data_ptr(), self._norm.data_ptr(), s),
                       "wavegrad_clip_adam")
            self._count("update", 2)
            if self.bf16:
                self._refresh(s)
                self._count("update")
        # the first read-back of the step: loss, overflow flag and norm
        loss, overflow = float(st.loss[0].item()), bool(int(self._flag[0].item()))
        self.last_norm = float(self._norm[0].item())
        self.scaler.update(overflow)
        if not overflow:
            self.steps += 1
        self.model._drop()  # the model's own operand copies are those of the old weights
        return loss, overflow, scale

    # ---- forward ----------------------------------------------------------------------------------------------------------------------
    def _forward(self, st, s):
        lib, ck = _lib.load(), _lib.check
        if self.bf16:
            ck(lib.ma_wavegrad_forward(ctypes.byref(st.c), st.audio.data_ptr(), st.mel.data_ptr(), st.enc.data_ptr(), st.ld_enc,
                                       st.pred.data_ptr(), st.ws.data_ptr(), st.ws.numel(), s), "wavegrad_forward")
            self._count("forward", sum(st.B if d["kind"] in (_lib.WAVEGRAD_OP_CONV, _lib.WAVEGRAD_OP_DOWN) else 1 for d in st.ops))
            return
        B, base = st.B, st.ws.data_ptr()

        def at(name):
            return base + st.foff[name] if name is not None else None

        for op in st.ops:
            k, T = op["kind"], op["T"]
            if k == _lib.WAVEGRAD_OP_INIT:
                ck(lib.ma_wavegrad_init_conv_f32(st.audio.data_ptr(), B, T, op["w"].data_ptr(), op["bias"].data_ptr(), op["taps"], op["N"],
                                                 at(op["out"]), s), "init_conv")
                self._count("forward")
            elif k == _lib.WAVEGRAD_OP_PACK:
                x = st.mel.data_ptr() if op["inp"] == _lib.WAVEGRAD_BUF_MEL else at(op["inp"])
                enc = st.enc.data_ptr() + op["enc_off"] * 4 if op["enc_off"] >= 0 else None
                ck(lib.ma_wavegrad_pack_f32(x, B, T // op["f"], op["f"], op["C"], op["halo"], at(op["in2"]), op["ld_film"], enc, st.ld_enc,
                                            op["slope"], op["mul"], at(op["out"]), at(op["out2"]), op["res_mul"], s), "pack_f32")
                self._count("forward")
            elif k == _lib.WAVEGRAD_OP_CONV:
                n, c, taps, d, h = op["N"], op["Cpad"], op["taps"], op["dilation"], op["halo"]
                rows_u, w = T + 2 * h, op["w"].data_ptr()
                for b in range(B):
                    out = at(op["out"]) + b * T * n * 4
                    res = at(op["residual"]) + b * T * n * 4 if op.get("residual") is not None else None
                    for j in range(taps):
                        a = at(op["inp"]) + ((b * rows_u + h + (j - taps // 2) * d) * c) * 4
                        e = _epilogue(op["alpha"], op["bias"].data_ptr(), res, n) if j == 0 else _epilogue(op["alpha"], None, out, n)
                        ck(lib.ma_gemm_x32(a, c, 1, w + j * c * 4, taps * c, 1, out, n, T, n, c, ctypes.byref(e), s), "gemm_x32 conv")
                self._count("forward", B * taps)
            elif k == _lib.WAVEGRAD_OP_DOWN:
                n, c, f, h = op["N"], op["Cpad"], op["f"], op["halo"]
                rows_u, e = T * f + 2 * h, _epilogue(1.0, op["bias"].data_ptr())
                for b in range(B):
                    a = at(op["inp"]) + ((b * rows_u + h) * c) * 4
                    ck(lib.ma_gemm_x32(a, f * c, 1, op["w"].data_ptr(), f * c, 1, at(op["out"]) + b * T * n * 4, n, T, n, f * c,
                                       ctypes.byref(e), s), "gemm_x32 down")
                self._count("forward", B)
            else:
                ck(lib.ma_wavegrad_last_conv_update_f32(at(op["inp"]), B, T, op["C"], op["w"].data_ptr(), op["bias"].data_ptr(), op["taps"],
                                                        None, None, 0.0, 0.0, 0.0, None, st.pred.data_ptr(), s), "last_conv")
                self._count("forward")

    # ---- backward ---------------------------------------------------------------------------------------------------------------------
    def _backward(self, st, s):
        lib, ck, bf, B = _lib.load(), _lib.check, self.bf16, st.B
        fbase, gbase, gimg = st.ws.data_ptr(), st.gws.data_ptr(), st.gimg.data_ptr()
        seen = set()

        def at(name):
            return fbase + st.foff[name] if name is not None else None

        def gat(name):
            return gbase + st.goff[name]

        def width(c):
            return _pad64(c) if bf else c

        def gslot(name, leaf):
            return self.params.ptr(name + leaf, self.params.grad)

        def grad_image(op, halo):
            """The operand image of the gradient of op's output (slope 1, mul = alpha): one image serves dX and dW."""
            n, T = op["N"], op["T"]
            if bf:
                ck(lib.ma_wavegrad_pack_bf16(gat(op["out"]), B, T, 1, n, _pad64(n), halo, None, 0, None, 0, 1.0, op["alpha"], gimg, None, 0.0,
                                             s), "grad image")
            else:
                ck(lib.ma_wavegrad_pack_f32(gat(op["out"]), B, T, 1, n, halo, None, 0, None, 0, 1.0, op["alpha"], gimg, None, 0.0, s),
                   "grad image")
            self._count("backward")

        for op in reversed(st.ops):
            k, T = op["kind"], op["T"]
            if k == _lib.WAVEGRAD_OP_LAST:
                ck(lib.ma_wavegrad_l1_last_bwd_f32(st.pred.data_ptr(), st.noise.data_ptr(), at(op["inp"]), B, T, op["C"], op["w"].data_ptr(),
                                                   op["taps"], self.scaler.scale, st.g.data_ptr(), gat(op["inp"]), st.last_part.data_ptr(),
                                                   st.last_stride, st.loss_part.data_ptr(), st.loss.data_ptr(), s), "l1_last_bwd")
                seen.add(op["inp"])
                self._count("backward", 2)
            elif k == _lib.WAVEGRAD_OP_CONV:
                name, n, c, taps = self._by_ptr[op["w"].data_ptr()]
                d, h, cp, np_ = op["dilation"], op["halo"], width(c), width(op["N"])
                if op.get("residual") is not None:
                    seen.add(op["residual"])  # (the same buffer as the output's gradient)
                grad_image(op, h)
                rows_u = T + 2 * h
                tn = (st.tn_ws.data_ptr(), st.tn_bytes) if bf else (None, 0)
                self._count("backward", conv_dw(lib, bf, gimg, np_, at(op["inp"]), cp, gslot(name, ".weight"), gslot(name, ".bias"), n, c, taps,
                                                d, B * rows_u, tn[0], tn[1], s))
                img = st.images[op["inp"]]
                if img["inp"] != _lib.WAVEGRAD_BUF_MEL:  # dX, added to what other consumers of the operand left
                    w = self._rev[name].data_ptr() if bf else op["w"].data_ptr()
                    self._count("backward", conv_dx(lib, bf, gimg, np_, w, gat(op["inp"]), st.rowlen[op["inp"]][1], op["inp"] in seen, B, T, h,
                                                    n, c, taps, d, s))
                    seen.add(op["inp"])
            elif k == _lib.WAVEGRAD_OP_DOWN:
                name, n, c, f = self._by_ptr[op["w"].data_ptr()]
                h, cp, np_ = op["halo"], width(c), width(op["N"])
                grad_image(op, 0)
                assert st.rowlen[op["inp"]][1] == cp
                tn = (st.tn_ws.data_ptr(), st.tn_bytes) if bf else (None, 0)
                w = self._rev[name].data_ptr() if bf else op["w"].data_ptr()
                self._count("backward", down_bwd(lib, bf, gimg, np_, at(op["inp"]), cp, h, w, gat(op["inp"]), op["inp"] in seen,
                                                 gslot(name, ".weight"), gslot(name, ".bias"), B, T, n, c, f, tn[0], tn[1], s))
                seen.add(op["inp"])
            elif k == _lib.WAVEGRAD_OP_PACK:
                if op["inp"] == _lib.WAVEGRAD_BUF_MEL:
                    continue
                dop = gat(op["out"]) if op["out"] is not None and op["out"] in seen else None
                dres = gat(op["out2"]) if op["out2"] is not None and op["out2"] in seen else None
                film = op["in2"] if dop is not None else None
                ck(lib.ma_wavegrad_pack_bwd_f32(dop, st.rowlen[op["out"]][1] if dop is not None else 0, at(op["inp"]), B, T // op["f"], op["f"],
                                                op["C"], at(film), op["ld_film"] if film else 0, op["slope"], op["mul"], dres, op["res_mul"],
                                                gat(op["inp"]), 1 if op["inp"] in seen else 0, gat(film) if film else None,
                                                op["ld_film"] if film else 0, 1 if film in seen else 0, s), "pack_bwd")
                self._count("backward")
                seen.add(op["inp"])
                if film:
                    seen.add(film)
            else:  # INIT
                ck(lib.ma_wavegrad_init_conv_bwd_f32(gat(op["out"]), st.audio.data_ptr(), B, T, op["taps"], op["N"], st.init_part.data_ptr(), s),
                   "init_conv_bwd")
                self._count("backward")
        ck(lib.ma_reduce_splits_batch_f32(*st.reduce.args, s), "reduce_splits_batch")
        self._count("backward")
        self._act_grads = {"pred": st.g}
