"""WaveGrad on MI355X - mirror of mindaudio.models.wavegrad.WaveGrad (wavegrad_v190.py:174-241), forward only (the vocoder's
reverse loop is mindaudio_amd.wavegrad.reverse; training is models.wavegrad_train.WaveGradTrainer, on this forward).

Activations are time-major, channel-last float32.  Every convolution with more than one input channel is an MFMA product on bf16
operands: ma_conv1d_taps_bf16 for the plain / dilated "same" convolutions, ma_gemm_bf16 for the kernel = stride = factor downscales.
What sits between the products (the init convolution, the one operand producer with FiLM / LeakyReLU / encoding / repetition, the
last convolution fused with the diffusion update) is csrc/wavegrad.hip.  The network for one (B, frames) shape is a list of ops
(struct ma_wavegrad_op) over one workspace, filled here once per shape; ma_wavegrad_forward / ma_wavegrad_reverse walk it inside one
C call.  The rounding points are: both operands of every MFMA product are bf16, everything else (the init and last convolutions, the
FiLM arithmetic, the residual streams, the update) is float32.

PyTorch layers are parameter containers (their forward() is never called), named as the reference's cells so that checkpoint names
map one to one: DBlock.0, DBlock.n.{residual_dense, conv.1, conv.3, conv.5, downscale1, downscale2}, FiLM.n.{input_conv,
output_conv}, UBlock.n.{block1, block2_a, block2_b, block3_a, block3_b}, first_conv, last_conv."""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _host, _lib

__all__ = ["WaveGrad", "positional_table"]

_SQRT2 = math.sqrt(2.0)


def _get(obj, name):
    """hps.name for the reference's attribute object, hps["name"] for a (nested) dict."""
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def _pad64(c):
    return (c + 63) // 64 * 64


def positional_table(noise_levels, dims):
    """PositionalEncoding (wavegrad_v190.py:84-91) for every FiLM level as one host table: row s = concat over the levels of
    concat(sin(e), cos(e)), e = noise_levels[s] * exp(-ln(1e4) * i / count), count = dim // 2.  float64 arithmetic, rounded to
    float32.  -> ndarray (len(noise_levels), sum(dims)) float32."""
    nl = np.asarray(noise_levels, np.float64).reshape(-1, 1)
    parts = []
    for dim in dims:
        count = dim // 2
        e = nl * np.exp(-math.log(1e4) * (np.arange(count, dtype=np.float64) / count))[None, :]
        parts += [np.sin(e), np.cos(e)]
    return np.concatenate(parts, axis=1).astype(np.float32)


def _conv(cin, cout, k, dilation=1, stride=1, orthogonal=True):
    conv = nn.Conv1d(cin, cout, k, stride=stride, dilation=dilation)  # (padding is the kernels' business: forward() is never called)
    if orthogonal:
        nn.init.orthogonal_(conv.weight)  # Conv1dOrthogonal (wavegrad_v190.py:12-16)
    else:
        nn.init.xavier_uniform_(conv.weight)
    nn.init.zeros_(conv.bias)  # MindSpore's default bias_init
    return conv


class _DBlock(nn.Module):
    def __init__(self, cin, hidden, factor, kernels, dilations):
        super().__init__()
        self.factor = factor
        self.residual_dense = _conv(cin, hidden, 1)
        self.conv = nn.Sequential(
            nn.LeakyReLU(0.2), _conv(cin, hidden, kernels[0], dilations[0]), nn.LeakyReLU(0.2),
            _conv(hidden, hidden, kernels[1], dilations[1]), nn.LeakyReLU(0.2), _conv(hidden, hidden, kernels[2], dilations[2]))
        self.downscale1 = _conv(hidden, hidden, factor, stride=factor, orthogonal=False)
        self.downscale2 = _conv(cin, cin, factor, stride=factor, orthogonal=False)


class _FiLM(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.input_conv = _conv(cin, cin, k, orthogonal=False)
        self.output_conv = _conv(cin, 2 * cout, k, orthogonal=False)


class _UBlock(nn.Module):
    def __init__(self, cin, hidden, factor, k, dilation):
        super().__init__()
        self.factor, self.dilation = factor, list(dilation)
        self.block1 = _conv(cin, hidden, 1)
        self.block2_a = _conv(cin, hidden, k, dilation[0])
        self.block2_b = _conv(hidden, hidden, k, dilation[1])
        self.block3_a = _conv(hidden, hidden, k, dilation[2])
        self.block3_b = _conv(hidden, hidden, k, dilation[3])


class _Plan:
    """The op list of one (B, frames) shape, its workspace and everything they point to (kept alive here)."""


class WaveGrad(nn.Module):
    """WaveGrad(hps): the reference's one argument, an object with the attributes of wavegrad_base.yaml (dblock, film, ublock,
    first_conv, n_mels, hop_samples); a nested dict is accepted as well.

    Not built (NotImplementedError, raised before any device call): even kernel sizes, a FiLM kernel other than 3 (the reference pads
    it by 1 whatever its size), init / last kernels above 7, channel counts that are no multiples of 8, list lengths that do not
    chain: film.output_size[n-1] == dblock.hidden_size[n-1], reversed film.output_size == ublock.hidden_size, every DBlock
    resolution equal to the matching UBlock's, hop_samples == prod(ublock.factor).  The reference builds its downscales with kernel
    = stride = factor, and so does this class; a channel count that is no multiple of 64 is padded with zero columns.

    forward(noisy_audio (B, T) float32, noise_scale (B,) or (1,), spectrogram (B, n_mels, T / hop) float32) -> (B, T) float32 on the
    device; ValueError for T != hop * frames, a CPU tensor or a wrong rank."""

    def __init__(self, hps):
        super().__init__()
        db, fl, ub, fc = _get(hps, "dblock"), _get(hps, "film"), _get(hps, "ublock"), _get(hps, "first_conv")
        c0, k0 = int(_get(db, "init_conv_channels")), int(_get(db, "init_conv_kernels"))
        d_hidden, d_factor = list(_get(db, "hidden_size")), list(_get(db, "factor"))
        d_kernels, d_dil = list(_get(db, "kernel_size")), list(_get(db, "dilations"))
        f_out, f_k = list(_get(fl, "output_size")), list(_get(fl, "kernel_size"))
        u_hidden, u_factor, u_dil = list(_get(ub, "hidden_size")), list(_get(ub, "factor")), [list(d) for d in _get(ub, "dilation")]
        u_k = int(_get(ub, "kernel_size"))
        first_hidden, first_k = int(_get(fc, "hidden_size")), int(_get(fc, "kernel_size"))
        n_mels, hop = int(_get(hps, "n_mels")), int(_get(hps, "hop_samples"))

        kernels = [k0, u_k, first_k] + d_kernels + f_k
        if any(k % 2 == 0 or k < 1 for k in kernels):
            raise NotImplementedError("an even kernel size changes the sequence length under pad_mode='same'; not built")
        if any(k != 3 for k in f_k):
            raise NotImplementedError("the FiLM convolutions are built for kernel_size 3 (the reference pads them by 1)")
        if k0 > 7 or first_k > 7:
            raise NotImplementedError("the init and last convolutions are built for kernels up to 7")
        L = len(f_out)
        if len(d_hidden) != len(d_factor) or len(f_k) != L or len(d_hidden) != L - 1 or len(u_hidden) != L or len(u_factor) != L or \
                len(u_dil) != L or len(d_kernels) != 3 or len(d_dil) != 3 or any(len(d) != 4 for d in u_dil):
            raise NotImplementedError("the dblock / film / ublock lists do not chain (lengths)")
        if any(f_out[n - 1] != d_hidden[n - 1] for n in range(1, L)):
            raise NotImplementedError("film.output_size[n-1] must equal dblock.hidden_size[n-1]")
        if f_out[::-1] != u_hidden:
            raise NotImplementedError("reversed film.output_size must equal ublock.hidden_size")
        if any(math.prod(u_factor[j + 1:]) != math.prod(d_factor[:L - 1 - j]) for j in range(L)):
            raise NotImplementedError("every DBlock resolution must equal the matching UBlock's")
        if math.prod(u_factor) != hop:
            raise NotImplementedError("hop_samples must equal the product of ublock.factor")
        if any(c % 8 or c < 8 for c in [c0, n_mels, first_hidden] + d_hidden + f_out):
            raise NotImplementedError("channel counts must be multiples of 8 (16-byte rows)")
        if min(d_factor + u_factor + d_dil + [d for dl in u_dil for d in dl]) < 1:
            raise ValueError("factors and dilations must be positive")

        self.n_mels, self.hop, self.levels = n_mels, hop, L
        self.halo = max([(k // 2) * d for k, d in zip(d_kernels, d_dil)] + [(u_k // 2) * d for dl in u_dil for d in dl] +
                        [first_k // 2, 1])
        self.DBlock = nn.ModuleList([_conv(1, c0, k0)])
        cin = c0
        for hidden, factor in zip(d_hidden, d_factor):
            self.DBlock.append(_DBlock(cin, hidden, factor, d_kernels, d_dil))
            cin = hidden
        self.FiLM = nn.ModuleList()
        cin = c0
        self.enc_dims = []
        for cout, k in zip(f_out, f_k):
            self.FiLM.append(_FiLM(cin, cout, k))
            self.enc_dims.append(cin)
            cin = cout
        self.UBlock = nn.ModuleList()
        cin = first_hidden
        for hidden, factor, dil in zip(u_hidden, u_factor, u_dil):
            self.UBlock.append(_UBlock(cin, hidden, factor, u_k, dil))
            cin = hidden
        self.first_conv = _conv(n_mels, first_hidden, first_k)
        self.last_conv = _conv(u_hidden[-1], 1, first_k)  # (the reference takes first_conv.kernel_size here: wavegrad_v190.py:224)
        self._prepared = None
        self._plans = {}
        # any load_state_dict invalidates the bf16 / padded copies of prepare() and the plans that point to them (as ConvTasNet does)
        self.register_load_state_dict_post_hook(lambda module, _keys: module._drop())

    def _drop(self):
        self._prepared = None
        self._plans = {}

    # ---- weights ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self):
        """The operand copies: Conv1d weights (N, C, k) -> (N, k, Cpad) bf16 with zero columns C .. Cpad - 1 (the same layout serves
        the kernel = stride = f downscales as (N, f, Cpad)), biases float32, the init / last weights transposed float32."""
        self._plans = {}

        def mfma(conv, pad_rows=False):
            w = conv.weight.detach().to(torch.float32)
            n, c, k = w.shape
            npad = _pad64(n) if pad_rows else n
            out = torch.zeros((npad, k, _pad64(c)), dtype=torch.float32, device=w.device)
            out[:n, :, :c] = w.permute(0, 2, 1)
            b = torch.zeros((npad,), dtype=torch.float32, device=w.device)
            b[:n] = conv.bias.detach().to(torch.float32)
            return out.to(torch.bfloat16).contiguous(), b

        P = {id(m): mfma(m) for m in self.modules() if isinstance(m, nn.Conv1d) and m not in (self.DBlock[0], self.last_conv)}
        for blk in list(self.DBlock)[1:]:
            P[id(blk.residual_dense)] = mfma(blk.residual_dense, pad_rows=True)  # its bf16 output is the downscale's operand
        i, l = self.DBlock[0], self.last_conv
        P["init"] = (i.weight.detach().to(torch.float32)[:, 0, :].t().contiguous(), i.bias.detach().to(torch.float32).contiguous())
        P["last"] = (l.weight.detach().to(torch.float32)[0].t().contiguous(), l.bias.detach().to(torch.float32).contiguous())
        self._prepared = P
        return self

    # ---- the plan ---------------------------------------------------------------------------------------------------------------------
    def _build_ops(self, B, frames):
        """-> (ops as dicts with buffer NAMES, {name: bytes}).  Buffers: see struct ma_wavegrad_op."""
        P, h, T = self._prepared, self.halo, self.hop * frames
        ops, sizes = [], {}
        counter = [0]

        def new(nbytes):
            counter[0] += 1
            name = "b%d" % counter[0]
            sizes[name] = nbytes
            return name

        def pack(x, t_out, c, f=1, film=None, enc_off=-1, slope=1.0, mul=1.0, want_out=True, res_mul=None, halo=h, once=0):
            out = new(B * (t_out + 2 * halo) * _pad64(c) * 2) if want_out else None
            res = new(B * t_out * c * 4) if res_mul is not None else None
            ops.append(dict(kind=_lib.WAVEGRAD_OP_PACK, once=once, inp=x, in2=film[0] if film else None, out=out, out2=res, T=t_out,
                            ld_film=film[1] if film else 0, C=c, Cpad=_pad64(c), f=f, halo=halo, enc_off=enc_off, slope=slope, mul=mul,
                            res_mul=res_mul or 0.0))
            return out, res

        def conv(op_in, t, conv_mod, residual=None, alpha=1.0, out_bf16=False, once=0, halo=h):
            w, b = P[id(conv_mod)]
            n, taps, cpad = w.shape
            out = new(B * t * n * (2 if out_bf16 else 4))
            ops.append(dict(kind=_lib.WAVEGRAD_OP_CONV, once=once, inp=op_in, out=out, residual=residual, w=w, bias=b, T=t, Cpad=cpad, N=n,
                            taps=taps, dilation=conv_mod.dilation[0], halo=halo, out_bf16=int(out_bf16), alpha=alpha))
            return out

        def down(op_in, t_out, conv_mod, halo):
            w, b = P[id(conv_mod)]
            n, f, cpad = w.shape
            out = new(B * t_out * n * 4)
            ops.append(dict(kind=_lib.WAVEGRAD_OP_DOWN, inp=op_in, out=out, w=w, bias=b, T=t_out, Cpad=cpad, N=n, f=f, halo=halo, alpha=1.0))
            return out

        # DBlocks and FiLMs (wavegrad_v190.py:228-232)
        c = self.DBlock[0].out_channels
        x = new(B * T * c * 4)
        ops.append(dict(kind=_lib.WAVEGRAD_OP_INIT, inp=_lib.WAVEGRAD_BUF_AUDIO, out=x, w=P["init"][0], bias=P["init"][1], T=T, N=c,
                        taps=self.DBlock[0].kernel_size[0]))
        t, enc_off, films = T, 0, []
        for n, film in enumerate(self.FiLM):
            opx, _ = pack(x, t, c)  # serves FiLM.input_conv and the next DBlock's residual_dense / downscale2
            hid = conv(opx, t, film.input_conv)
            oph, _ = pack(hid, t, c, slope=0.2, enc_off=enc_off)
            enc_off += c
            cout = film.output_conv.out_channels // 2
            films.append((conv(oph, t, film.output_conv), 2 * cout, cout, t))
            if n + 1 < len(self.DBlock):
                blk = self.DBlock[n + 1]
                f, hidden = blk.factor, blk.residual_dense.out_channels
                r1 = conv(opx, t, blk.residual_dense, out_bf16=True)  # (B, t, pad64(hidden)) bf16, no halo: the downscale reads no tap
                res = down(r1, t // f, blk.downscale1, halo=0)
                y = down(opx, t // f, blk.downscale2, halo=h)
                t //= f
                for i, cm in enumerate((blk.conv[1], blk.conv[3], blk.conv[5])):
                    op_y, _ = pack(y, t, cm.in_channels, slope=0.2)
                    y = conv(op_y, t, cm, residual=res if i == 2 else None)
                x, c = y, hidden
        # first_conv and the UBlocks (:234-237)
        opm, _ = pack(_lib.WAVEGRAD_BUF_MEL, frames, self.n_mels, once=1)
        x, c, t = conv(opm, frames, self.first_conv, once=1), self.first_conv.out_channels, frames
        for blk, (fbuf, ld, cout, t_film) in zip(self.UBlock, films[::-1]):
            f, hidden = blk.factor, blk.block1.out_channels
            assert t * f == t_film and cout == hidden
            film = (fbuf, ld)
            op1, _ = pack(x, t, c)
            b1 = conv(op1, t, blk.block1)
            _, r1 = pack(b1, t * f, hidden, f=f, want_out=False, res_mul=1.0 / (f * _SQRT2))      # block1 repeated / f / sqrt 2
            op2, _ = pack(x, t * f, c, f=f, slope=0.2, mul=1.0 / f)
            t *= f
            a = conv(op2, t, blk.block2_a)
            opa, _ = pack(a, t, hidden, film=film, slope=0.2)
            y = conv(opa, t, blk.block2_b, residual=r1, alpha=1.0 / _SQRT2)                        # (block1 + block2) / sqrt 2
            opy, r2 = pack(y, t, hidden, film=film, slope=0.2, res_mul=1.0 / _SQRT2)
            cc = conv(opy, t, blk.block3_a)
            opc, _ = pack(cc, t, hidden, film=film, slope=0.2)
            x, c = conv(opc, t, blk.block3_b, residual=r2, alpha=1.0 / _SQRT2), hidden              # (x + block3) / sqrt 2
        ops.append(dict(kind=_lib.WAVEGRAD_OP_LAST, inp=x, w=P["last"][0], bias=P["last"][1], T=t, C=c, taps=self.last_conv.kernel_size[0]))
        assert t == T
        return ops, sizes

    @staticmethod
    def _allocate(ops, sizes):
        """Byte offsets by liveness: a buffer's block is free again after its last reader.  A step defines every buffer before it
        reads it, so the order inside one step decides; what a `once` op touches keeps a block of its own for the whole call."""
        roles = ("inp", "in2", "out", "out2", "residual")
        last, pinned = {}, set()
        for i, op in enumerate(ops):
            for r in roles:
                name = op.get(r)
                if isinstance(name, str):
                    last[name] = i
                    if op.get("once"):
                        pinned.add(name)
        offsets, free, top = {}, [], 0
        for i, op in enumerate(ops):
            for r in ("out", "out2"):
                name = op.get(r)
                if isinstance(name, str) and name not in offsets:
                    need = (sizes[name] + 255) // 256 * 256
                    fit = [blk for blk in free if blk[0] >= need] if name not in pinned else []
                    if fit:
                        blk = min(fit)
                        free.remove(blk)
                        offsets[name] = blk
                    else:
                        offsets[name] = (need, top)
                        top += need
            for name in {op.get(r) for r in roles}:
                if isinstance(name, str) and last[name] == i and name not in pinned:
                    free.append(offsets[name])
        return {k: v[1] for k, v in offsets.items()}, top

    def _plan(self, B, frames, dev):
        key = (B, frames, str(dev))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        if len(self._plans) >= 4:
            self._plans.clear()
        ops, sizes = self._build_ops(B, frames)
        offsets, _top = self._allocate(ops, sizes)
        arr = (_lib.WaveGradOp * len(ops))()

        def off(v):
            if v is None:
                return _lib.WAVEGRAD_BUF_NONE
            return offsets[v] if isinstance(v, str) else v

        for o, d in zip(arr, ops):
            o.kind, o.once = d["kind"], d.get("once", 0)
            o.inp, o.in2, o.out, o.out2, o.residual = (off(d.get(r)) for r in ("inp", "in2", "out", "out2", "residual"))
            o.w = d["w"].data_ptr() if d.get("w") is not None else None
            o.bias = d["bias"].data_ptr() if d.get("bias") is not None else None
            o.T, o.ld_film = d["T"], d.get("ld_film", 0)
            o.C, o.Cpad, o.N, o.taps, o.dilation = d.get("C", 0), d.get("Cpad", 0), d.get("N", 0), d.get("taps", 1), d.get("dilation", 1)
            o.f, o.halo, o.out_bf16, o.enc_off = d.get("f", 1), d.get("halo", 0), d.get("out_bf16", 0), d.get("enc_off", -1)
            o.slope, o.mul, o.res_mul, o.alpha = d.get("slope", 1.0), d.get("mul", 1.0), d.get("res_mul", 0.0), d.get("alpha", 1.0)
        plan = _Plan()
        plan.ops, plan.n_launches = arr, sum(B if d["kind"] in (_lib.WAVEGRAD_OP_CONV, _lib.WAVEGRAD_OP_DOWN) else 1
                                             for d in ops if not d.get("once"))
        plan.c = _lib.WaveGradPlan(len(ops), sum(self.enc_dims), B, self.hop * frames, frames, self.n_mels, arr)
        nbytes = _lib.load().ma_wavegrad_workspace_bytes(ctypes.byref(plan.c))
        if nbytes < 0:
            _lib.check(int(nbytes), "wavegrad plan")
        plan.ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)
        plan.ws_bytes = int(nbytes)
        self._plans[key] = plan
        return plan

    # ---- calls --------------------------------------------------------------------------------------------------------------------------
    def _check_inputs(self, audio, spectrogram):
        if audio.dim() != 2 or spectrogram.dim() != 3:
            raise ValueError("noisy_audio must be (B, T) and spectrogram (B, n_mels, frames)")
        B, T = audio.shape
        if spectrogram.shape[0] != B or spectrogram.shape[1] != self.n_mels:
            raise ValueError("spectrogram must be (B, n_mels, frames) with the audio's batch size")
        frames = spectrogram.shape[2]
        if frames < 1 or T != self.hop * frames:
            raise ValueError("T must equal hop_samples * frames (%d * %d), got %d" % (self.hop, frames, T))
        if not audio.is_cuda or not spectrogram.is_cuda:
            raise ValueError("the inputs must be tensors on the HIP device (there is no CPU path)")
        if self.last_conv.weight.device != audio.device:
            raise ValueError("the inputs and the model's parameters are on different devices")
        return B, T, frames

    def _ready(self, dev):
        _host.require_gpu()
        if self._prepared is None or self._prepared["last"][0].device != dev:
            self.prepare()

    @staticmethod
    def mel_rows(spectrogram):
        """(B, n_mels, frames) -> the time-major (B, frames, n_mels) float32 copy the kernels read."""
        return spectrogram.to(torch.float32).transpose(1, 2).contiguous()

    @torch.no_grad()
    def forward(self, noisy_audio, noise_scale, spectrogram):
        B, T, frames = self._check_inputs(noisy_audio, spectrogram)
        levels = np.asarray(noise_scale.detach().cpu() if torch.is_tensor(noise_scale) else noise_scale, np.float64).reshape(-1)
        if levels.size not in (1, B):
            raise ValueError("noise_scale must hold one value, or one per utterance")
        dev = noisy_audio.device
        self._ready(dev)
        plan = self._plan(B, frames, dev)
        enc = torch.from_numpy(positional_table(levels, self.enc_dims)).to(dev)
        audio = noisy_audio.to(torch.float32).contiguous()
        mel = self.mel_rows(spectrogram)
        pred = torch.empty((B, T), dtype=torch.float32, device=dev)
        with _host.pinned_stream():
            _lib.check(_lib.load().ma_wavegrad_forward(ctypes.byref(plan.c), audio.data_ptr(), mel.data_ptr(), enc.data_ptr(),
                                                       enc.shape[1] if levels.size > 1 else 0, pred.data_ptr(), plan.ws.data_ptr(),
                                                       plan.ws_bytes, _host.current_stream_ptr()), "wavegrad_forward")
        return pred

    @torch.no_grad()
    def reverse_steps(self, audio, mel_rows, enc_table, c1, c2, sigma, noise, first_step, n_steps):
        """Iterations first_step .. first_step + n_steps - 1 of the reverse loop in one C call (ma_wavegrad_reverse), `audio` (B, T)
        float32 updated in place.  mel_rows = WaveGrad.mel_rows(spectrogram); enc_table (S, sum(enc_dims)) float32 on the device;
        c1, c2, sigma float32 host arrays [S]; noise (n_steps, B, T) float32 on the device (None when the only step is the last)."""
        B, T = audio.shape
        frames = mel_rows.shape[1]
        if T != self.hop * frames or mel_rows.shape != (B, frames, self.n_mels):
            raise ValueError("audio (B, hop * frames) and mel_rows (B, frames, n_mels) do not match")
        if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous():
            raise ValueError("audio must be a contiguous float32 tensor on the HIP device")
        S = len(c1)
        n_noise = n_steps - 1 if first_step + n_steps == S else n_steps
        if n_noise > 0 and (noise is None or noise.shape[0] < n_noise or tuple(noise.shape[1:]) != (B, T)):
            raise ValueError("noise must hold one (B, T) draw per step with n > 0")
        dev = audio.device
        self._ready(dev)
        plan = self._plan(B, frames, dev)
        fp = ctypes.POINTER(ctypes.c_float)
        c1, c2, sigma = (np.ascontiguousarray(v, np.float32) for v in (c1, c2, sigma))
        with _host.pinned_stream():
            _lib.check(_lib.load().ma_wavegrad_reverse(
                ctypes.byref(plan.c), audio.data_ptr(), mel_rows.data_ptr(), enc_table.data_ptr(), c1.ctypes.data_as(fp),
                c2.ctypes.data_as(fp), sigma.ctypes.data_as(fp), noise.data_ptr() if noise is not None else None, S, first_step, n_steps,
                plan.ws.data_ptr(), plan.ws_bytes, _host.current_stream_ptr()), "wavegrad_reverse")
        return audio

    def launches_per_step(self, B, frames):
        """Kernel launches of one loop iteration for this shape (the MFMA products run once per utterance)."""
        dev = self.last_conv.weight.device
        self._ready(dev)
        return self._plan(B, frames, dev).n_launches
