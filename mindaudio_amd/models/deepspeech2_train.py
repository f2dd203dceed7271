"""DeepSpeech2 training step on MI355X: examples/deepspeech2/train.py around mindaudio/models/deepspeech2.py - NetWithCTCLoss,
TrainOneStepWithLossScaleCell and nn.Adam.  frontend="frozen" (the default) trains the recurrent stack and fc: the convolution front end
(MaskConv) runs as DeepSpeechModel.frontend runs it, BatchNorm as the folded inference affine.  frontend="trained" trains conv1, conv2
and both BatchNorm2d as well, as the reference does (below).  `train_conv=True` raises NotImplementedError: use frontend="trained".

  forward   model.frontend, then per layer ma_lstm_bidir_train_bf16 (ma_lstm_bidir_bf16's launches plus the tape), then the fc GEMM of
            DeepSpeechModel.forward: the logits have the bits of model.forward.
  loss      NetWithCTCLoss: softmax inside the loss, blank = len(labels) - 1 (the yaml's "_"), mean over the batch:
            ma_ctc_loss_grad_f32 with grad_scale = loss_scale / B and zero_infinity = 1.  The logits are time-major and the CTC entry
            reads batch-major rows: the 29-column logits and dlogits are reordered by a torch copy each.
  backward  fc: dW = ma_gemm_tn_bf16_f32(dlogits, h), dh = ma_gemm_bf16 on the transposed weight.  Per layer, top down:
            ops.lstm_bidir_backward (ma_lstm_bidir_bwd_bf16, one launch per time step, then dW_ih / db / dW_hh / dx from dgates by the
            library's products).  The bf16 rounding of a layer's output is passed straight through: a layer's dx is the dout of the
            layer below.  Layer 0 computes no dx (frozen front end).
  update    ma_grad_overflow_f32 over the flat gradient, ma_adam_f32 over the flat parameters and moments (skipped on the device when
            the flag is set), then one re-pack per layer.

What the reference's script does and this keeps (each measured against a float64 restatement in tests/test_deepspeech2_train_gpu.py):
  * the scale sense is the constant Tensor(1024): it is never adjusted, an overflow only skips the update;
  * Adam(..., loss_scale=1024) divides the already unscaled gradient by 1024 a second time: inv_scale = 1 / (loss_scale *
    optimizer_loss_scale).  Adam's step is scale-free except for eps, so in effect eps is 1024 times larger;
  * step_lr is computed and never used: the rate is constant;
  * the yaml's weight_decay and momentum are unused.
What it does not keep: the data set pads every target row to 350 entries with the blank id and passes all 350 as labels; this trainer
takes the true lengths.  Targets longer than 223 labels are beyond ma_ctc_loss_grad_f32 and raise ValueError.

The trained parameters, their gradient and both moments are a train.flat.FlatParams (8-element alignment) in the reference's layouts;
the model's parameters become views of it.  Layer 0's weight_ih is kept in the reference's c * F2 + f
column order; the kernels' f * 32 + c order exists only in the packed operands, and its gradient is permuted back.

frontend="trained" (csrc/deepspeech2_train.hip, ops.ds2_frontend_train / ops.ds2_frontend_backward).  The flat store also holds
conv.conv1.weight (32, 1, 41, 11), conv.conv2.weight (32, 32, 21, 11) and conv.bn{1,2}.gamma / beta in the reference's names and
shapes; Adam and the overflow check stay one launch each.
  forward   conv1 raw (float32 y1 and per-workgroup double partials) -> batch statistics -> tanh(BatchNorm) as the bf16 act1 image;
            conv2 per output frequency with a plain float32 epilogue -> batch statistics -> tanh(BatchNorm) as the bf16 LSTM input.
            Nothing is masked, as in the reference: padded frames enter the statistics.  The logits differ from model.forward's by
            design (batch statistics instead of the moving ones).
  backward  layer 0 also computes dx = d loss / d xin; BatchNorm + tanh backward, conv2's weight gradient (ma_gemm_tn_bf16_f32 per time
            tap and output frequency), conv2's input gradient (ma_conv1d_taps_bf16 per input frequency on transposed weights),
            BatchNorm + tanh backward again, conv1's weight gradient (a direct float32 kernel).
  moving statistics  moving = 0.9 * moving + 0.1 * batch (MindSpore's momentum=0.9), the UNBIASED batch variance for moving_variance
            and the biased one for normalising.  That MindSpore uses the unbiased one there is restated from its documentation of
            BatchNorm2d, not verified against MindSpore.  The forward writes the new values to a copy; loss_and_grads never touches
            the model's, and step commits the copy on the device only if the step's overflow flag is clear (ma_ds2_commit_f32).
  Not kept: the reference's BatchNorm updates its moving statistics inside the forward, so an overflowing step (a NaN input) poisons
            them for good; here a skipped step leaves them as they were.
  After a committed step the model's folded inference operands are marked stale and re-derived by the next model.frontend()."""
import ctypes

import numpy as np
import torch

from .. import _host, _lib, ops
from ..train import kernels
from ..train.flat import ADAM_BETA1, ADAM_BETA2, FlatTrainer, adam_lr_t
from . import _lstm
from .deepspeech2 import DeepSpeechModel, permute_wih_columns

__all__ = ["DeepSpeech2Trainer", "unpermute_wih_columns", "MAX_TARGET_LENGTH"]

_F32, _BF16 = torch.float32, torch.bfloat16
MAX_TARGET_LENGTH = 223  # ma_ctc_loss_grad_f32: 2 L + 1 <= 448 lattice states
_LEAVES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def unpermute_wih_columns(w, channels, n_freq):
    """The inverse of permute_wih_columns: (4H, n_freq * channels) with column f * channels + c -> column c * n_freq + f."""
    w = torch.as_tensor(w)
    return w.reshape(w.shape[0], n_freq, channels).permute(0, 2, 1).reshape(w.shape[0], channels * n_freq)


class DeepSpeech2Trainer(FlatTrainer):
    """DeepSpeech2Trainer(model, learning_rate, eps, loss_scale=1024, optimizer_loss_scale=None, train_conv=False, frontend="frozen").

    loss_and_grads(x (B, 1, F, T), lengths (B), targets (B, Lmax) int32, target_lengths (B)) -> loss (float): the mean over the batch
        of the CTC losses; gradients() then holds d(loss_scale * loss) / d parameter under the reference's names and layouts.
    step(x, lengths, targets, target_lengths) -> (loss, overflow): the same, then nn.Adam on gradient / (loss_scale *
        optimizer_loss_scale); a non-finite gradient sets `overflow` and leaves parameters and moments untouched.
    state_dict() / load_state_dict(): the model's entries plus "moment1.<name>", "moment2.<name>" and "steps".
    optimizer_loss_scale defaults to loss_scale (the yaml's OptimConfig.loss_scale next to Tensor(1024)).
    frontend: "frozen" trains the recurrent stack and fc; "trained" also conv1, conv2 and both BatchNorm2d, with batch statistics in
        the forward (`logits` then differs from model.forward's) and the moving statistics advanced by every step that is not skipped."""

    def __init__(self, model, learning_rate, eps, loss_scale=1024, optimizer_loss_scale=None, train_conv=False, frontend="frozen"):
        if train_conv:
            raise NotImplementedError('train_conv is not an option of this trainer: pass frontend="trained" to train MaskConv')
        if frontend not in ("frozen", "trained"):
            raise ValueError('frontend must be "frozen" or "trained", got %r' % (frontend,))
        self.frontend = frontend
        if not isinstance(model, DeepSpeechModel):
            raise TypeError("model must be a models.DeepSpeechModel")
        if not learning_rate > 0 or not eps > 0 or not loss_scale > 0:
            raise ValueError("learning_rate, eps and loss_scale must be positive")
        self.model, self.learning_rate, self.eps = model, float(learning_rate), float(eps)
        self.loss_scale = float(loss_scale)
        self.optimizer_loss_scale = self.loss_scale if optimizer_loss_scale is None else float(optimizer_loss_scale)
        self.blank = len(model.labels) - 1
        self.steps = 0
        self.launches = {}  # the library's launches per phase of the last step (torch's copies and fills are not counted)
        self.logits = None
        self._fe_tape = None  # (frontend="trained": the front end's tape of the last forward, until step has committed its statistics)
        self.events = None  # a list: every phase boundary of a step appends (name, torch.cuda.Event) to it (tools/deepspeech2_train_bench.py)

    def _mark(self, name):
        if self.events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.events.append((name, ev))

    # ---- parameters ---------------------------------------------------------------------------------------------------------------
    def _names(self):
        out = []
        for k in range(self.model.hidden_layers):
            for suffix in ("", "_reverse"):
                out += ["RNN.lstms.%d.%s_l0%s" % (k, leaf, suffix) for leaf in _LEAVES]
        out += ["fc.module.weight"]
        if self.frontend == "trained":
            out += ["conv.conv1.weight", "conv.bn1.gamma", "conv.bn1.beta", "conv.conv2.weight", "conv.bn2.gamma", "conv.bn2.beta"]
        return out

    def _bind(self, dev):
        shapes = {name: tuple(p.shape) for name, p in self.model.named_parameters()}
        self._bind_params([(name, shapes[name]) for name in self._names()], dev, mirror_bf16=False, moments=("moment1", "moment2"))
        self._flag = torch.zeros(4, dtype=torch.int32, device=dev)
        self.model._prepared = None
        if self.frontend == "trained":  # the four moving-statistics vectors as views of ONE buffer: a step commits them in one launch
            self._moving = torch.empty(128, dtype=_F32, device=dev)
            c = self.model.conv
            for i, p in enumerate((c.bn1.moving_mean, c.bn1.moving_variance, c.bn2.moving_mean, c.bn2.moving_variance)):
                view = self._moving[32 * i:32 * i + 32]
                view.copy_(p.detach().to(dev, _F32))
                p.data = view

    def _repack(self):
        """The operands of every layer and of fc from the float32 masters: one pack per layer (csrc/lstm.hip, csrc/lstm_train.hip)."""
        m = self.model
        if m._prepared is None:
            m.prepare()  # (the frozen front end's operands; its layers are replaced below)
        P, H = m._prepared, m.hidden_size
        layers = []
        for k in range(m.hidden_layers):
            fwd, bwd = ([self.params.p("RNN.lstms.%d.%s_l0%s" % (k, leaf, d)) for leaf in _LEAVES] for d in ("", "_reverse"))
            if k == 0:
                fwd[0], bwd[0] = permute_wih_columns(fwd[0], 32, m.F2), permute_wih_columns(bwd[0], 32, m.F2)
            layers.append(_lstm.pack_bidir_train_layer(fwd, bwd, m.rnn_input_size if k == 0 else H, H))
        P["layers"] = layers
        fc = self.params.p("fc.module.weight")
        P["fc"] = fc.to(_BF16).contiguous()
        C = fc.shape[0]
        fct = torch.zeros((H, _lstm.ceil64(C)), dtype=_BF16, device=fc.device)  # dh = dlogits (rows, 64) . fc: W (N = H, K = 64)
        fct[:, :C] = P["fc"].t()
        P["fc_t"] = fct
        if self.frontend == "trained":
            P["frontend_train"] = ops.ds2_frontend_operands(m)
            P["frontend_stale"] = True  # (the folded inference operands: DeepSpeechModel.frontend re-derives them when it next runs)

    # ---- calls ----------------------------------------------------------------------------------------------------------------------
    def _count(self, phase, n=1):
        self.launches[phase] = self.launches.get(phase, 0) + n

    def _check_targets(self, B, targets, target_lengths):
        tl = np.asarray(target_lengths.detach().cpu() if torch.is_tensor(target_lengths) else target_lengths).astype(np.int64).reshape(-1)
        if tl.shape != (B,) or tl.min() < 0:
            raise ValueError("target_lengths must hold one non-negative length per utterance")
        if tl.max() > MAX_TARGET_LENGTH:
            raise ValueError("a target of %d labels: ma_ctc_loss_grad_f32 takes at most %d" % (tl.max(), MAX_TARGET_LENGTH))
        ys = torch.as_tensor(np.asarray(targets.detach().cpu()) if torch.is_tensor(targets) else np.asarray(targets))
        if ys.dim() != 2 or ys.shape[0] != B or ys.shape[1] < tl.max() or ys.is_floating_point():
            raise ValueError("targets must be a (B, Lmax) integer array with Lmax >= max(target_lengths)")
        L = max(1, int(tl.max()))
        ys = ys[:, :L] if ys.shape[1] >= L else torch.zeros((B, L), dtype=torch.int32)
        if ys.numel() and (int(ys.min()) < 0 or int(ys.max()) >= len(self.model.labels)):
            raise ValueError("targets must be label ids")
        return ys.to(torch.int32).contiguous(), torch.from_numpy(tl.astype(np.int32))

    def loss_and_grads(self, x, lengths, targets, target_lengths):
        return float(self._run(x, lengths, targets, target_lengths).item())

    def _run(self, x, lengths, targets, target_lengths):
        m = self.model
        B = x.shape[0]
        ys, ylens = self._check_targets(B, targets, target_lengths)
        _host.require_gpu()
        dev = m.fc.module.weight.device
        if dev.type != "cuda":
            raise ValueError("the model's parameters must be on the HIP device (there is no CPU path)")
        lib, ck = _lib.load(), _lib.check
        self.launches = {}
        with torch.no_grad():
            if self.params is None:
                self._bind(dev)
            elif self.params.master.device != dev:
                raise ValueError("the trainer is bound to %s" % self.params.master.device)
            if m._prepared is None or "whh_bwd" not in m._prepared["layers"][0]:
                self._repack()
            P, H, C = m._prepared, m.hidden_size, len(m.labels)
            out_len = torch.from_numpy(m.get_seq_lens(lengths).astype(np.int32))
            # ---- forward
            self._mark("start")
            trained = self.frontend == "trained"
            if trained:
                xin, self._fe_tape = ops.ds2_frontend_train(m, x, P["frontend_train"], mark=self._mark if self.events is not None else None)
                self._count("forward", 4 + m.F2 + 3)
            else:
                xin = m.frontend(x)
                self._count("forward", 1 + m.F2)
            T1 = xin.shape[0]
            _, hb, tapes = _lstm.run_train_layers(P["layers"], xin)
            chunks = -(-T1 // max(1, min(T1, (1 << 26) // (B * 4 * H))))  # (ops.lstm_bidir_train's projection chunks)
            self._count("forward", len(tapes) * (2 + 2 * chunks + T1 + (T1 & 1)))  # fills, projections, steps and the odd-T join
            ldc = (C + 7) // 8 * 8
            logits = torch.empty((T1, B, ldc), dtype=_F32, device=dev)
            e = _lib.GemmEpilogue()
            e.alpha, e.act, e.act2, e.out_bf16 = 1.0, _lib.ACT_NONE, _lib.ACT_NONE, 0
            s = _host.current_stream_ptr()
            ck(lib.ma_gemm_bf16(hb.data_ptr(), H, P["fc"].data_ptr(), H, logits.data_ptr(), ldc, T1 * B, C, H, ctypes.byref(e), s), "ds2_fc")
            self._count("forward")
            self.logits = logits[:, :, :C]
            self._mark("forward")
            # ---- loss: batch-major rows of 64 columns, so that dlogits is a K-padded GEMM operand
            ld = _lstm.ceil64(C)
            rows = torch.zeros((B, T1, ld), dtype=_F32, device=dev)
            rows[:, :, :C] = self.logits.permute(1, 0, 2)
            loss, _per, dlog = kernels.ctc_loss_grad(rows.view(B * T1, ld), C, B, T1, ys.to(dev), out_len.to(dev), ylens.to(dev),
                                                     self.loss_scale / B, blank=self.blank)
            dlog = dlog.view(B, T1, ld).permute(1, 0, 2).contiguous().view(T1 * B, ld)  # back to time-major rows
            self._count("loss", 4)
            self._mark("loss")
            # ---- backward
            self.params.grad.zero_()
            g = self.gradients()
            tnb = int(lib.ma_gemm_tn_workspace_bytes(ld, H, T1 * B))
            tn = torch.empty((tnb + 256,), dtype=torch.uint8, device=dev)
            dfc = torch.empty((ld, H), dtype=_F32, device=dev)
            ck(lib.ma_gemm_tn_bf16_f32(dlog.data_ptr(), ld, hb.data_ptr(), H, dfc.data_ptr(), H, ld, H, T1 * B, C, 1.0, 0, None, tn.data_ptr(),
                                       tnb, s), "ds2 dW_fc")
            g["fc.module.weight"].copy_(dfc[:C])
            dh = torch.empty((T1, B, H), dtype=_F32, device=dev)
            ck(lib.ma_gemm_bf16(dlog.data_ptr(), ld, P["fc_t"].data_ptr(), ld, dh.data_ptr(), H, T1 * B, H, ld, ctypes.byref(e), s), "ds2 dh")
            self._count("backward", 4)
            for k in range(m.hidden_layers - 1, -1, -1):
                L = P["layers"][k]
                res = ops.lstm_bidir_backward(dh, tapes[k], L, need_dx=k > 0 or trained)
                tapes[k] = None  # (the tape is the largest buffer of the step: let it go as soon as it has been read)
                # one fill, the steps, per direction dW_ih + db (3 launches) and dW_hh (2), and the two dx products
                self._count("backward", 1 + T1 + 2 * (3 + (2 if T1 > 1 else 0)) + (2 if k > 0 or trained else 0))
                for d, suffix in enumerate(("", "_reverse")):
                    pre = "RNN.lstms.%d." % k
                    dw = res["dw_ih"][d][:, :L["K"]]
                    g[pre + "weight_ih_l0" + suffix].copy_(unpermute_wih_columns(dw, 32, m.F2) if k == 0 else dw)
                    g[pre + "weight_hh_l0" + suffix].copy_(res["dw_hh"][d])
                    g[pre + "bias_ih_l0" + suffix].copy_(res["db"][d])
                    g[pre + "bias_hh_l0" + suffix].copy_(res["db"][d])
                if k > 0:
                    dh = res["dx"][:, :, :H] if L["Kpad"] != H else res["dx"]
                    dh = dh.contiguous()
            if trained:
                self._mark("lstm_backward")
                fe = ops.ds2_frontend_backward(res["dx"], self._fe_tape, mark=self._mark if self.events is not None else None)
                for name, n in fe["launches"].items():
                    self._count("frontend_" + name, n)
                for name in ("conv.conv1.weight", "conv.bn1.gamma", "conv.bn1.beta", "conv.conv2.weight", "conv.bn2.gamma", "conv.bn2.beta"):
                    g[name].copy_(fe[name])
            self._mark("backward")
        return loss

    def step(self, x, lengths, targets, target_lengths):
        loss = self._run(x, lengths, targets, target_lengths)
        fp = self.params
        lr_t = adam_lr_t(self.learning_rate, self.steps + 1, ADAM_BETA1, ADAM_BETA2)
        with torch.no_grad():
            self._flag.zero_()
            kernels.grad_overflow(fp.grad, self._flag)
            kernels.adam(fp.master, fp.grad, fp.moment1, fp.moment2, lr_t, ADAM_BETA1, ADAM_BETA2, self.eps,
                         1.0 / (self.loss_scale * self.optimizer_loss_scale), overflow=self._flag)
            self._count("update", 2)
            if self.frontend == "trained":  # the new moving statistics, unless the step is skipped: decided on the device
                _lib.check(_lib.load().ma_ds2_commit_f32(self._moving.data_ptr(), self._fe_tape.moving.data_ptr(), 128, self._flag.data_ptr(),
                                                         _host.current_stream_ptr()), "ds2_commit")
                self._count("update")
                self._fe_tape = None
            overflow = bool(int(self._flag[0].item()))  # the step's read-back, with the loss
            loss = float(loss.item())
            if not overflow:
                self.steps += 1
                self._repack()
                self._count("update", 3 * self.model.hidden_layers)
            self._mark("update")
        return loss, overflow
