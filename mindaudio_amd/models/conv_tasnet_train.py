"""Conv-TasNet training step on MI355X: the forward that keeps what the backward reads, the PIT SI-SNR gradient, the hand-written
backward and nn.SGD (examples/conv_tasnet/train.py:80-110 around mindaudio/models/conv_tasnet.py and separation_loss.py).

The products are the library's GEMMs - ma_gemm_bf16 for the forward and, on a transposed weight copy, for dX (the residual stream's
gradient rides in its residual epilogue), ma_gemm_tn_bf16_f32 for dW = dY^T X; everything between them is a kernel of
csrc/conv_tasnet_train.hip (float32 with whole-utterance float64 sums, per-workgroup partials joined in a fixed order, no atomics).
`operands="f32"` is the validation mode: the same kernels, every product through ma_gemm_x32 on float32 activations and weights.

The parameters, the gradients, the momentum buffers and the bf16 mirror are a train.flat.FlatParams (8-element alignment), so the
optimizer is one launch.  The model's parameters become views of its masters; the depthwise and the
encoder weights are kept in the forward kernels' transposed order ((P, H) and (L, N)) and the model sees transposed views, so no
layout copy runs in a step.  Moving the model to another device after the trainer has bound it is not supported.

Per block the forward keeps: the operand image of the block input, the conv1x1 output before PReLU, the depthwise output before PReLU,
both statistics partials and the operand image of the second gLN's output - 5632 bytes per frame and block in bf16 mode."""
import ctypes

import torch

from .. import _host, _lib, ops
from ..train import plans
from ..train.flat import FlatTrainer, stored_last_first
from .conv_tasnet import _OVERLAP, ConvTasNet, _epilogue

__all__ = ["ConvTasNetTrainer"]

_TRAIN_H = (64, 128, 256, 512, 1024)  # one channel group per thread in the depthwise backward
_OUTER_MAX = 12288                    # L * N of the basis / encoder gradient kernels


class ConvTasNetTrainer(FlatTrainer):
    """ConvTasNetTrainer(model, momentum=0.0, weight_decay=0.0, operands="bf16", overlap=model.overlap).

    loss_and_grads(mixture (M, T), sources (M, C, T_out), lengths) -> loss (float); one float32 gradient per parameter, under the names
        of model.state_dict(), is then in gradients().  T_out = (K + 1) L / 2 must equal the sources' length.
    step(mixture, sources, lengths, lr) -> loss; the same plus the SGD update (g += wd p; buf = g on the first step, else
        momentum buf + g; p -= lr buf), the refresh of the bf16 and transposed weight copies, and the inference copies invalidated.
    state_dict() / load_state_dict(): the model's entries plus "momentum.<name>" and "steps".

    Not built (NotImplementedError before any device call): H outside {64, 128, 256, 512, 1024}, L * N > 12288, C > 8."""

    def __init__(self, model, momentum=0.0, weight_decay=0.0, operands="bf16", overlap=None):
        if not isinstance(model, ConvTasNet):
            raise TypeError("model must be a models.ConvTasNet")
        if operands not in ("bf16", "f32"):
            raise ValueError("operands must be 'bf16' or 'f32'")
        overlap = model.overlap if overlap is None else overlap
        if overlap not in _OVERLAP:
            raise ValueError("overlap must be 'paired' or 'true'")
        if momentum < 0 or weight_decay < 0:
            raise ValueError("momentum and weight_decay must not be negative")
        if model.H not in _TRAIN_H:
            raise NotImplementedError("the depthwise backward is built for H in %s" % (_TRAIN_H,))
        if model.L * model.N > _OUTER_MAX:
            raise NotImplementedError("the basis / encoder gradient kernels are built for L * N <= %d" % _OUTER_MAX)
        if model.C > 8:
            raise NotImplementedError("the SI-SNR gradient is built for at most 8 sources")
        self.model, self.momentum, self.weight_decay = model, float(momentum), float(weight_decay)
        self.operands, self.overlap, self.bf16 = operands, overlap, operands == "bf16"
        self.steps = 0
        self._ws = {}
        self._stale = True
        model.register_load_state_dict_post_hook(lambda module, _keys: setattr(self, "_stale", True))

    # ---- parameters ---------------------------------------------------------------------------------------------------------------
    def _bind(self, dev):
        m = self.model
        tap_major = ("depthwise_conv.weight", "conv1d_U.weight")  # kept (P, H) and (L, N), the order the forward kernels read
        self._bind_params([(name, tuple(p.shape), stored_last_first if name.endswith(tap_major) else None) for name, p in m.named_parameters()],
                          dev, mirror_bf16=self.bf16, moments=("momentum",) if self.momentum > 0 else ())
        fp, f32 = self.params, torch.float32
        self._one = torch.ones(4, dtype=f32, device=dev)
        # the 1 x 1 convolutions: (out, in) views of the float32 master, the bf16 mirror and a transposed bf16 copy for dX
        self._w1x1 = [n for n in fp.index if n.endswith(("conv1x1.weight", "pointwise_conv.weight"))]
        self._wt = {}
        if self.bf16:
            tot = sum((fp.index[n][2] + 7) // 8 * 8 for n in self._w1x1)
            self._wt_flat = torch.zeros(tot, dtype=torch.bfloat16, device=dev)
            o, items = 0, []
            for n in self._w1x1:
                rows, cols = fp.index[n][1][:2]
                self._wt[n] = self._wt_flat[o:o + rows * cols].view(cols, rows)
                o += (rows * cols + 7) // 8 * 8
                w = self._w(n, bf=True)
                items.append((_lib.TransposeItem(w.data_ptr(), self._wt[n].data_ptr(), cols, rows, rows, cols, 0, (cols + 63) // 64),
                              ((rows + 63) // 64) * ((cols + 63) // 64)))
            self._wt_plan = plans.ItemTable(items, dev)
        m._prepared = None
        self._stale = True

    def _w(self, name, bf=False):
        off, shape, n = self.params.index[name]
        src = self.params.bf16 if bf else self.params.master
        return src[off:off + n].view(shape[0], shape[1])

    def _refresh(self, s):
        """The bf16 mirror and the transposed copies from the float32 master (after a load; a step refreshes them itself)."""
        lib = _lib.load()
        if self.bf16:
            _lib.check(lib.ma_cast_f32_bf16(self.params.master.data_ptr(), self.params.bf16.data_ptr(), self.params.size, s), "cast")
            _lib.check(lib.ma_transpose_batch_bf16(*self._wt_plan.args, s), "transpose_batch")
        self._stale = False

    def activation_gradients(self):
        """The gradients of the last backward at the estimate, the mask scores, the bottleneck output and the normalised mixture_w."""
        return dict(self._act_grads)

    # ---- workspaces -----------------------------------------------------------------------------------------------------------------
    def _workspace(self, M, T, K, dev):
        key = (M, T)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        if len(self._ws) >= 2:
            self._ws.clear()
        m, lib = self.model, _lib.load()
        N, L, B, H, C = m.N, m.L, m.B, m.H, m.C
        nblk, rows, f32 = len(m.blocks()), M * K, torch.float32
        opd = torch.bfloat16 if self.bf16 else f32

        def e(cols, dtype=f32):
            return torch.empty((rows, cols), dtype=dtype, device=dev)

        tn, th = lib.ma_tasnet_stat_parts(K, N), lib.ma_tasnet_stat_parts(K, H)
        gd, ge = lib.ma_tasnet_decode_bwd_parts(K, C, N, L), lib.ma_tasnet_encode_bwd_parts(K, N, L)
        if min(tn, th, gd, ge) < 1:
            raise NotImplementedError("shape outside the training kernels' limits")

        def f64(n):
            return torch.empty(n, dtype=torch.float64, device=dev)

        ws = dict(tn=tn, th=th, mw=e(N), nb=e(N, opd), part_n=f64(M * tn * 3), y0=[e(H) for _ in range(nblk)], d0=[e(H) for _ in range(nblk)],
                  hop=[e(H, opd) for _ in range(nblk)], part_a=[f64(M * th * 3) for _ in range(nblk)],
                  part_b=[f64(M * th * 3) for _ in range(nblk)], p1=e(H), z=e(H), score=e(C * N),
                  out=torch.empty((M, C, (K + 1) * (L // 2)), dtype=f32, device=dev))
        if self.bf16:  # the float32 residual stream ping-pongs; its bf16 image is kept per block
            ws["x"], ws["xop"] = (e(B), e(B)), [e(B, opd) for _ in range(nblk + 1)]
        else:          # float32 operands: the stream itself is kept per block
            ws["xop"] = [e(B) for _ in range(nblk + 1)]
        # backward
        ws.update(d_est=torch.empty_like(ws["out"]), d_score=e(C * N), dmw=e(N), dx=(e(B), e(B)), dh=e(H), du=e(H), dy0=e(H, opd), dnb=e(N),
                  p2h=f64(M * th * 2), p2u=f64(M * th * 2), p2n=f64(M * tn * 2))
        if self.bf16:
            ws["d_score_op"], ws["dx_op"] = e(C * N, opd), e(B, opd)
            nbytes = max(int(lib.ma_gemm_tn_workspace_bytes(mo, no, rows)) for mo, no in ((B, N), (H, B), (B, H), (C * N, B)))
            ws["tn_ws"], ws["tn_bytes"] = torch.empty(nbytes // 4 + 4, dtype=f32, device=dev), nbytes
        # parameter-gradient partials, and the one launch that sums them all in a fixed order
        sizes = [M * th, M * th, M * th * 3 * H] * nblk + [M * gd * L * N, M * ge * L * N]
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 7) // 8 * 8
        arena = ws["parts"] = torch.empty(tot, dtype=f32, device=dev)
        base, items = arena.data_ptr(), []

        def item(i, name, mn, splits):
            off = self.params.index[name][0]
            items.append(plans._reduce_item(base + offs[i] * 4, self.params.grad[off:off + mn], mn, mn, mn, splits, mn, splits >= 64, accumulate=False))
            return base + offs[i] * 4

        names = self._block_names()
        ws["pp"] = []
        for b in range(nblk):
            ws["pp"].append((item(3 * b, names[b]["a1"], 1, M * th), item(3 * b + 1, names[b]["a2"], 1, M * th),
                             item(3 * b + 2, names[b]["dw"], 3 * H, M * th)))
        ws["pp_basis"] = item(3 * nblk, "decoder.basis_signals.weight", L * N, M * gd)
        ws["pp_enc"] = item(3 * nblk + 1, "encoder.conv1d_U.weight", L * N, M * ge)
        ws["reduce"] = plans.ItemTable(items, dev)
        self._ws[key] = ws
        return ws

    def _block_names(self):
        out = []
        for r in range(self.model.R):
            for x in range(self.model.X):
                p = "separator.temporal_conv_net.%d.%d." % (r, x)
                out.append(dict(c1=p + "conv1x1.weight", a1=p + "prelu.weight", dw=p + "dsconv.depthwise_conv.weight",
                                a2=p + "dsconv.prelu.weight", pw=p + "dsconv.pointwise_conv.weight", d=2 ** x))
        return out

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    def _check_inputs(self, mixture, sources, lengths):
        m = self.model
        if mixture.dim() != 2 or sources.dim() != 3 or sources.shape[0] != mixture.shape[0] or sources.shape[1] != m.C:
            raise ValueError("mixture must be (M, T) and sources (M, C, T)")
        M, T = mixture.shape
        if T < m.L:
            raise ValueError("mixture shorter than one encoder filter (T < L)")
        K = m.num_frames(T)
        if sources.shape[2] != (K + 1) * (m.L // 2):
            raise ValueError("the sources must have the estimate's length (K + 1) L / 2 = %d" % ((K + 1) * (m.L // 2)))
        if not mixture.is_cuda or not sources.is_cuda:
            raise ValueError("mixture and sources must be tensors on the HIP device (there is no CPU path)")
        if len(lengths) != M:
            raise ValueError("one length per utterance")
        return M, T, K

    def loss_and_grads(self, mixture, sources, lengths):
        M, T, K = self._check_inputs(mixture, sources, lengths)
        _host.require_gpu()
        dev = mixture.device
        with torch.no_grad():
            if self.params is None:
                self.model.to(dev)
                self._bind(dev)
            elif self.params.master.device != dev:
                raise ValueError("the trainer is bound to %s" % self.params.master.device)
            ws = self._workspace(M, T, K, dev)
            x_in = mixture.to(torch.float32).contiguous()
            src = sources.to(torch.float32).contiguous()
            lens = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64)
            with _host.pinned_stream():
                s = _host.current_stream_ptr()
                if self._stale:
                    self._refresh(s)
                self._forward(ws, x_in, M, T, K, s)
            loss, _, _, perm, _ = ops.si_snr_pit(src, ws["out"], lens)
            with _host.pinned_stream():
                s = _host.current_stream_ptr()
                self._backward(ws, x_in, src, lens, perm.contiguous(), M, T, K, s)
            return float(loss)

    def step(self, mixture, sources, lengths, lr):
        loss = self.loss_and_grads(mixture, sources, lengths)
        lib, fp = _lib.load(), self.params
        with torch.no_grad(), _host.pinned_stream():
            s = _host.current_stream_ptr()
            _lib.check(lib.ma_sgd_momentum_f32(fp.master.data_ptr(), fp.grad.data_ptr(),
                                               fp.momentum.data_ptr() if self.momentum > 0 else None, fp.size, float(lr),
                                               self.momentum, self.weight_decay, 1 if self.steps == 0 else 0,
                                               fp.bf16.data_ptr() if self.bf16 else None, s), "sgd_momentum")
            if self.bf16:
                _lib.check(lib.ma_transpose_batch_bf16(*self._wt_plan.args, s), "transpose_batch")
        self.steps += 1
        self.model._prepared = None
        return loss

    def _gemms(self, rows, ws, s):
        lib, ck, bf, ptr = _lib.load(), _lib.check, self.bf16, self.params.ptr

        def shape(name):
            return self.params.index[name][1][:2]  # (out, in)

        def fwd(a, name, out, residual=None):
            n, k = shape(name)
            epi = _epilogue(residual.data_ptr(), n) if residual is not None else _epilogue()
            if bf:
                ck(lib.ma_gemm_bf16(a.data_ptr(), k, self._w(name, True).data_ptr(), k, out.data_ptr(), n, rows, n, k, ctypes.byref(epi), s),
                   "gemm")
            else:
                ck(lib.ma_gemm_x32(a.data_ptr(), k, 1, ptr(name), k, 1, out.data_ptr(), n, rows, n, k, ctypes.byref(epi), s), "gemm_x32")

        def dx(dy, name, out, residual=None):  # out (rows, in) = dy (rows, out) . W (+ residual)
            n, k = shape(name)
            epi = _epilogue(residual.data_ptr(), k) if residual is not None else _epilogue()
            if bf:
                ck(lib.ma_gemm_bf16(dy.data_ptr(), n, self._wt[name].data_ptr(), n, out.data_ptr(), k, rows, k, n, ctypes.byref(epi), s),
                   "gemm dX")
            else:
                ck(lib.ma_gemm_x32(dy.data_ptr(), n, 1, ptr(name), 1, k, out.data_ptr(), k, rows, k, n, ctypes.byref(epi), s),
                   "gemm_x32 dX")

        def dw(dy, x, name):  # grad (out, in) = dy^T . x
            n, k = shape(name)
            g = ptr(name, self.params.grad)
            if bf:
                ck(lib.ma_gemm_tn_bf16_f32(dy.data_ptr(), n, x.data_ptr(), k, g, k, n, k, rows, n, 1.0, 0, None, ws["tn_ws"].data_ptr(),
                                           ws["tn_bytes"], s), "gemm dW")
            else:
                ck(lib.ma_gemm_x32(dy.data_ptr(), 1, n, x.data_ptr(), 1, k, g, k, n, k, rows, None, s), "gemm_x32 dW")

        return fwd, dx, dw

    def _forward(self, ws, x_in, M, T, K, s):
        m, lib, ck, bf, ptr = self.model, _lib.load(), _lib.check, self.bf16, self.params.ptr
        N, L, B, H, C = m.N, m.L, m.B, m.H, m.C
        rows = M * K
        fwd, _, _ = self._gemms(rows, ws, s)
        norm = lib.ma_gln_apply_bf16 if bf else lib.ma_gln_apply_f32
        mw, pn = ws["mw"], ws["part_n"].data_ptr()
        ck(lib.ma_tasnet_encode_f32(x_in.data_ptr(), M, T, T, ptr("encoder.conv1d_U.weight"), L, N, mw.data_ptr(), pn, s),
           "tasnet_encode")
        ck(norm(mw.data_ptr(), M, K, N, pn, ws["nb"].data_ptr(), s), "gln_apply")
        names = self._block_names()
        cur = ws["x"][0] if bf else ws["xop"][0]
        fwd(ws["nb"], "separator.bottleneck_conv1x1.weight", cur)
        for b, nm in enumerate(names):
            if bf:
                ck(lib.ma_cast_f32_bf16(cur.data_ptr(), ws["xop"][b].data_ptr(), rows * B, s), "cast")
            y0, d0, pa, pb = ws["y0"][b], ws["d0"][b], ws["part_a"][b].data_ptr(), ws["part_b"][b].data_ptr()
            fwd(ws["xop"][b], nm["c1"], y0)
            ck(lib.ma_prelu_gln_stats(y0.data_ptr(), M, K, H, ptr(nm["a1"]), ws["p1"].data_ptr(), pa, s), "prelu_gln_stats")
            ck(lib.ma_gln_dwconv_prelu_train(ws["p1"].data_ptr(), M, K, H, pa, ptr(nm["dw"]), m.P, nm["d"], ptr(nm["a2"]),
                                             d0.data_ptr(), ws["z"].data_ptr(), pb, s), "gln_dwconv_prelu_train")
            ck(norm(ws["z"].data_ptr(), M, K, H, pb, ws["hop"][b].data_ptr(), s), "gln_apply")
            nxt = ws["x"][(b + 1) % 2] if bf else ws["xop"][b + 1]
            fwd(ws["hop"][b], nm["pw"], nxt, residual=cur)
            cur = nxt
        if bf:
            ck(lib.ma_cast_f32_bf16(cur.data_ptr(), ws["xop"][-1].data_ptr(), rows * B, s), "cast")
        fwd(ws["xop"][-1], "separator.mask_conv1x1.weight", ws["score"])
        ck(lib.ma_tasnet_decode_f32(ws["score"].data_ptr(), mw.data_ptr(), M, K, C, N, ptr("decoder.basis_signals.weight"), L,
                                    _OVERLAP[self.overlap], ws["out"].data_ptr(), s), "tasnet_decode")

    def _backward(self, ws, x_in, src, lens, perm, M, T, K, s):
        m, lib, ck, bf, ptr = self.model, _lib.load(), _lib.check, self.bf16, self.params.ptr
        N, L, B, H, C = m.N, m.L, m.B, m.H, m.C
        rows = M * K
        _, dx, dw = self._gemms(rows, ws, s)
        names = self._block_names()

        def operand(t, op):  # the GEMM operand image of a float32 gradient
            if not bf:
                return t
            ck(lib.ma_cast_f32_bf16(t.data_ptr(), op.data_ptr(), t.numel(), s), "cast")
            return op

        ck(lib.ma_si_snr_grad_f32(src.data_ptr(), ws["out"].data_ptr(), lens.data_ptr(), perm.data_ptr(), M, C, src.shape[2],
                                  ws["d_est"].data_ptr(), s), "si_snr_grad")
        ck(lib.ma_tasnet_decode_bwd_f32(ws["d_est"].data_ptr(), ws["score"].data_ptr(), ws["mw"].data_ptr(), M, K, C, N,
                                        ptr("decoder.basis_signals.weight"), L, _OVERLAP[self.overlap], ws["d_score"].data_ptr(),
                                        ws["dmw"].data_ptr(), ws["pp_basis"], s), "tasnet_decode_bwd")
        ds = operand(ws["d_score"], ws.get("d_score_op"))
        dw(ds, ws["xop"][-1], "separator.mask_conv1x1.weight")
        cur, nxt = ws["dx"]
        dx(ds, "separator.mask_conv1x1.weight", cur)
        for b in range(len(names) - 1, -1, -1):
            nm = names[b]
            y0, d0, pa, pb = ws["y0"][b].data_ptr(), ws["d0"][b].data_ptr(), ws["part_a"][b].data_ptr(), ws["part_b"][b].data_ptr()
            pa1, pa2, pdw = ws["pp"][b]
            dxo = operand(cur, ws.get("dx_op"))
            dw(dxo, ws["hop"][b], nm["pw"])
            dx(dxo, nm["pw"], ws["dh"])
            ck(lib.ma_gln_bwd_stats(ws["dh"].data_ptr(), d0, M, K, H, pb, ptr(nm["a2"]), ws["p2h"].data_ptr(), s), "gln_bwd_stats")
            ck(lib.ma_gln2_bwd_dwconv(ws["dh"].data_ptr(), d0, y0, M, K, H, pa, pb, ws["p2h"].data_ptr(), ptr(nm["a1"]),
                                      ptr(nm["a2"]), ptr(nm["dw"]), m.P, nm["d"], ws["du"].data_ptr(), ws["p2u"].data_ptr(),
                                      pa2, pdw, s), "gln2_bwd_dwconv")
            ck(lib.ma_gln1_bwd(ws["du"].data_ptr(), y0, M, K, H, pa, ws["p2u"].data_ptr(), ptr(nm["a1"]), ws["dy0"].data_ptr(),
                               1 if bf else 0, pa1, s), "gln1_bwd")
            dw(ws["dy0"], ws["xop"][b], nm["c1"])
            dx(ws["dy0"], nm["c1"], nxt, residual=cur)  # d_x_in = d_x_out + d_conv1x1_out . W_c1
            cur, nxt = nxt, cur
        dxo = operand(cur, ws.get("dx_op"))
        dw(dxo, ws["nb"], "separator.bottleneck_conv1x1.weight")
        dx(dxo, "separator.bottleneck_conv1x1.weight", ws["dnb"])
        ck(lib.ma_gln_bwd_stats(ws["dnb"].data_ptr(), ws["mw"].data_ptr(), M, K, N, ws["part_n"].data_ptr(), self._one.data_ptr(),
                                ws["p2n"].data_ptr(), s), "gln_bwd_stats")
        ck(lib.ma_tasnet_encode_bwd_f32(x_in.data_ptr(), M, T, T, ws["mw"].data_ptr(), ws["part_n"].data_ptr(), ws["dnb"].data_ptr(),
                                        ws["p2n"].data_ptr(), ws["dmw"].data_ptr(), L, N, ws["pp_enc"], s), "tasnet_encode_bwd")
        ck(lib.ma_reduce_splits_batch_f32(*ws["reduce"].args, s), "reduce_splits_batch")
        self._act_grads = {"estimate": ws["d_est"], "score": ws["d_score"], "bottleneck": cur, "norm_mixture_w": ws["dnb"]}
