"""What the recurrent models share: the padding and time-chunk rules, the packing of one LSTM layer for either schedule
(csrc/lstm.hip, csrc/lstm_stack.hip), the layer loop over ma_lstm_bidir_bf16 with its buffers, and the loading of named weights."""
import numpy as np
import torch

from .. import _host, _lib


def ceil64(n):
    return (n + 63) // 64 * 64


def _pack(entry, what, src, K, H, **shapes):
    """One layer through a pack entry point whose outputs, in its argument order, have `shapes` (`bias` float32, the others bf16)."""
    L = {k: torch.empty(s, dtype=torch.float32 if k == "bias" else torch.bfloat16, device=src[0].device) for k, s in shapes.items()}
    _lib.check(entry(*[t.data_ptr() for t in src], K, ceil64(K), H, *[t.data_ptr() for t in L.values()], _host.current_stream_ptr()), what)
    torch.cuda.current_stream().synchronize()  # (the caller's `src` may go out of scope)
    return dict(L, Kpad=ceil64(K))


def pack_bidir_layer(fwd, bwd, K, H):
    """fwd, bwd = [weight_ih (4H, K), weight_hh (4H, H), bias_ih (4H), bias_hh (4H)] of a direction, float32 on the device ->
    ma_lstm_bidir_bf16's operands {wih, whh, bias, Kpad}.  bwd = None: a unidirectional layer for dir_mask = 1 (ma_lstm_pack_f32
    takes both directions stacked; the reverse half is zero and never run)."""
    src = [torch.stack([a, torch.zeros_like(a) if bwd is None else bwd[i]]).contiguous() for i, a in enumerate(fwd)]
    return _pack(_lib.load().ma_lstm_pack_f32, "lstm_pack", src, K, H, wih=(2, 4 * H, ceil64(K)), whh=(2 * 4 * H * H,), bias=(2, 4 * H))


def pack_bidir_train_layer(fwd, bwd, K, H):
    """pack_bidir_layer's operands plus what the backward pass reads: whh_bwd, W_hh in the backward step's fragment order
    (ma_lstm_pack_bwd_f32), and wih_t (2, Kpad, 4H) bf16, the transposed copy of wih for dx = dgates . W_ih."""
    L = pack_bidir_layer(fwd, bwd, K, H)
    w_hh = torch.stack([fwd[1], torch.zeros_like(fwd[1]) if bwd is None else bwd[1]]).contiguous()
    L["whh_bwd"] = torch.empty((2 * 4 * H * H,), dtype=torch.bfloat16, device=w_hh.device)
    _lib.check(_lib.load().ma_lstm_pack_bwd_f32(w_hh.data_ptr(), H, L["whh_bwd"].data_ptr(), _host.current_stream_ptr()), "lstm_pack_bwd")
    torch.cuda.current_stream().synchronize()  # (w_hh goes out of scope)
    L["wih_t"] = L["wih"].transpose(1, 2).contiguous()
    return dict(L, K=K)


def run_train_layers(layers, xin, ws=None):
    """The training forward of a stack of pack_bidir_train_layer's operands on a (T, B, Kpad) bf16 input, each layer reading the bf16
    output of the one below -> (float32 (T, B, H) and bf16 output of the last layer, [the layers' tapes]).  The same calls on the same
    operands as run_layers, so the outputs have its bits."""
    from .. import ops

    cur, tapes, of = xin, [], None
    for L in layers:
        of, cur, tape = ops.lstm_bidir_train(cur, L, workspace=ws)
        tapes.append(tape)
    return of, cur, tapes


def pack_stack_layer(src, K, H):
    """src = [weight_ih (4H, K), weight_hh (4H, H), bias_ih (4H), bias_hh (4H)] float32 on the device -> one layer of
    ma_lstm_stack_bf16's operands {packed, bias, Kpad}."""
    return _pack(_lib.load().ma_lstm_stack_pack_f32, "lstm_stack_pack", src, K, H, packed=(4 * H * (ceil64(K) + H),), bias=(4 * H,))


def layer_buffers(T, B, H, dev):
    """What run_layers needs for (T, B, H): the time chunk (frames per projection GEMM: a direction's float32 projection buffer holds
    at most 2^26 values), two float32 and two bf16 (T, B, H) outputs to alternate between, and the workspace."""
    chunk = max(1, min(T, (1 << 26) // (B * 4 * H)))
    nbytes = _lib.load().ma_lstm_workspace_bytes(T, B, H, chunk)
    if nbytes < 0:
        _lib.check(int(nbytes), "lstm_workspace_bytes")
    return dict(chunk=chunk, hf=[torch.empty((T, B, H), dtype=torch.float32, device=dev) for _ in range(2)],
                hb=[torch.empty((T, B, H), dtype=torch.bfloat16, device=dev) for _ in range(2)],
                lstm=torch.empty((int(nbytes),), dtype=torch.uint8, device=dev))


def run_layers(layers, xin, H, dir_mask, ws):
    """One ma_lstm_bidir_bf16 call per layer of pack_bidir_layer's operands on a (T, B, Kpad) bf16 input, each layer reading the
    bf16 output of the one below; ws: layer_buffers' entries.  -> (float32 (T, B, H), its bf16 rounding) of the last layer."""
    lib, (T, B, _), cur = _lib.load(), xin.shape, xin
    with _host.pinned_stream():
        s = _host.current_stream_ptr()
        for k, L in enumerate(layers):
            of, ob = ws["hf"][k & 1], ws["hb"][k & 1]
            _lib.check(lib.ma_lstm_bidir_bf16(cur.data_ptr(), T, B, L["Kpad"], H, L["wih"].data_ptr(), L["whh"].data_ptr(),
                                              L["bias"].data_ptr(), dir_mask, ws["chunk"], of.data_ptr(), ob.data_ptr(), None,
                                              ws["lstm"].data_ptr(), ws["lstm"].numel(), s), "lstm_bidir")
            cur = ob
    return of, ob


def load_named_weights(module, params, strict=True, reshape=False):
    """{the module's parameter name: array} -> the module's parameters, cast to their dtypes (and, with `reshape`, brought to their
    shapes).  -> (missing, unexpected); with `strict`, either one raises KeyError."""
    own = module.state_dict()
    state = {k: torch.as_tensor(np.asarray(v)).to(own[k].dtype) for k, v in params.items() if k in own}
    if reshape:
        state = {k: v.reshape(own[k].shape) for k, v in state.items()}
    missing = [k for k in own if k not in state]
    unexpected = [k for k in params if k not in own]
    if strict and (missing or unexpected):
        raise KeyError("parameters do not match the model: missing %s, unexpected %s" % (missing[:8], unexpected[:8]))
    module.load_state_dict(state, strict=False)
    return missing, unexpected
