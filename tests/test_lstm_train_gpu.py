"""GPU: one bidirectional LSTM layer's training step - ma_lstm_bidir_train_bf16 (csrc/lstm.hip's taping instantiations),
ma_lstm_pack_bwd_f32 / ma_lstm_bidir_bwd_bf16 (csrc/lstm_train.hip) and the products of ops.lstm_bidir_backward - against the float64
restatements and with the comparators of tests/lstm_train_cases.py, which tests/test_lstm_train_cases_cpu.py proves on the CPU.

Every kernel output (out_f32, out_bf16, the tape, dgates) sits in a sentinel-filled window between two sentinel-filled guard bands.
Shapes: H 64 / 128 are the forward's two step forms (and the backward's two operand-block sizes), K 40 / 64 with and without zero pad
columns, T 1 / 2 / 3 / 5 the first step and the odd-T tie, B 1 / 16 / 17 / 65 a partial tile, a second tile and a second workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import deepspeech2_cases as C
import lstm_train_cases as L

pytestmark = pytest.mark.gpu

GUARD = 256        # elements of a guard band (a multiple of 16 bytes for every dtype)
SENTINEL = -7.0    # float32 / bf16 windows
TAPE_FILL = 0x5A   # the tape is a byte buffer: 0x5A5A5A5A = 1.5e16 as float32, 0x5A5A = 1.5e16 as bf16

# (T, B, H, K, dir_mask): a pruned product of the shapes above
CASES = [(1, 1, 64, 40, 3), (2, 16, 128, 64, 3), (3, 17, 64, 64, 3), (5, 17, 64, 40, 3), (5, 65, 128, 40, 3), (1, 65, 64, 64, 3),
         (3, 16, 128, 40, 1), (2, 17, 64, 64, 2), (5, 1, 128, 64, 2)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    return _lib.load()


def _guarded(shape, dtype, fill=SENTINEL):
    n = int(np.prod(shape))
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return whole[GUARD:GUARD + n].view(*shape), whole


def _bands_untouched(whole, fill=SENTINEL):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _operands(x, layer):
    """-> (xb (T, B, Kpad) bf16 on the device, the packed layer of models._lstm.pack_bidir_train_layer)"""
    from mindaudio_amd.models import _lstm

    T, B, K = x.shape
    H = layer["weight_hh"].shape[2]
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    fwd, bwd = ([torch.from_numpy(np.ascontiguousarray(layer[n][d], dtype=np.float32)).cuda() for n in names] for d in (0, 1))
    xb = torch.zeros((T, B, _lstm.ceil64(K)), dtype=torch.bfloat16, device="cuda")
    xb[:, :, :K] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().to(torch.bfloat16)
    return xb, _lstm.pack_bidir_train_layer(fwd, bwd, K, H)


def _train_forward(lib, xb, P, dir_mask):
    """The training forward into guarded windows -> (out_f32, out_bf16, tape: ops.LstmTape, the three whole buffers)"""
    from mindaudio_amd import ops

    T, B, _ = xb.shape
    H = P["bias"].shape[1] // 4
    of, of_whole = _guarded((T, B, H), torch.float32)
    ob, ob_whole = _guarded((T, B, H), torch.bfloat16)
    tape_buf, tape_whole = _guarded((int(lib.ma_lstm_train_tape_bytes(T, B, H)),), torch.uint8, TAPE_FILL)
    of, ob, tape = ops.lstm_bidir_train(xb, P, dir_mask=dir_mask, chunk=2 if T > 2 else None, out_f32=of, out_bf16=ob, tape_buf=tape_buf)
    torch.cuda.synchronize()
    return of, ob, tape, (of_whole, ob_whole, tape_whole)


def _inference(lib, xb, P, dir_mask):
    from mindaudio_amd import _lib

    T, B, Kpad = xb.shape
    H = P["bias"].shape[1] // 4
    chunk = 2 if T > 2 else T
    nbytes = lib.ma_lstm_workspace_bytes(T, B, H, chunk)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    of = torch.full((T, B, H), SENTINEL, dtype=torch.float32, device="cuda")
    ob = torch.full((T, B, H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ma_lstm_bidir_bf16(xb.data_ptr(), T, B, Kpad, H, P["wih"].data_ptr(), P["whh"].data_ptr(), P["bias"].data_ptr(), dir_mask,
                                      chunk, of.data_ptr(), ob.data_ptr(), None, ws.data_ptr(), nbytes, s), "lstm")
    torch.cuda.synchronize()
    return of, ob


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


# ---- the training forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,H,K,dir_mask", CASES)
def test_forward_has_the_inference_bits_and_tapes_the_restatement(lib, T, B, H, K, dir_mask):
    x, layer, dout = L.make_case(T, B, H, K)
    xb, P = _operands(x, layer)
    of, ob, tape, wholes = _train_forward(lib, xb, P, dir_mask)
    ref_f, ref_b = _inference(lib, xb, P, dir_mask)
    assert torch.equal(_bits(of), _bits(ref_f)) and torch.equal(_bits(ob), _bits(ref_b))  # the same bits, not the same values
    assert _bands_untouched(wholes[0]) and _bands_untouched(wholes[1]) and _bands_untouched(wholes[2], TAPE_FILL)
    # a second run leaves the same bits everywhere
    of2, ob2, tape2, _ = _train_forward(lib, xb, P, dir_mask)
    assert torch.equal(_bits(of), _bits(of2)) and torch.equal(_bits(ob), _bits(ob2)) and torch.equal(tape.buf, tape2.buf)

    act, h = tape.views()
    exact = L.layer_step(x, layer, dout, dir_mask=dir_mask)
    rounded = L.layer_step(x, layer, dout, rounding=True, dir_mask=dir_mask)
    filled = int(np.frombuffer(bytes([TAPE_FILL] * 4), np.int32)[0])
    for d in (0, 1):
        if not dir_mask & (1 << d):  # a direction that does not run leaves its half of the tape alone
            assert bool((_bits(act[d]) == filled).all()) and bool((_bits(h[d]).view(torch.uint8) == TAPE_FILL).all())
            continue
        assert not bool((_bits(act[d]) == filled).any()), "an element of the tape was not written"
        got_act, got_h = act[d].double().cpu().numpy(), h[d].double().cpu().numpy()
        # the bound of the forward tests for the layer output (test_deepspeech2_gpu.py): relrms <= 2 S, S = the rounding points alone
        for name, got, want, rnd in [("i f g o c"[2 * q], got_act[:, q], exact["act"][d][:, q], rounded["act"][d][:, q]) for q in range(5)] + \
                                    [("h", got_h, exact["h"][d], rounded["h"][d])]:
            S, e = C.relrms(rnd, want), C.relrms(got, want)
            print("tape %s dir %d (T %d, B %d, H %d, K %d): relrms %.3e, rounding-only %.3e, ratio %.2f" % (name, d, T, B, H, K, e, S, e / S))
            assert 0 < S < 3e-2 and e <= 2 * S
        # the h image is the bf16 rounding of o tanh(c) of the float32 tape, up to the float32 evaluation of that product
        want_h = got_act[:, 3] * np.tanh(got_act[:, 4])
        assert np.abs(got_h - want_h).max() <= (2.0 ** -8 + 16 * L.U) * np.abs(want_h).max()


# ---- backward through time and the products -------------------------------------------------------------------------------------------------
def _backward(lib, xb, P, tape, dout, need_dx=True):
    from mindaudio_amd import ops

    T, B, H = tape.T, tape.B, tape.H
    dg, dg_whole = _guarded((2, T, B, 4 * H), torch.bfloat16)
    res = ops.lstm_bidir_backward(torch.from_numpy(np.ascontiguousarray(dout, dtype=np.float32)).cuda(), tape, P, need_dx=need_dx, dgates=dg)
    torch.cuda.synchronize()
    assert _bands_untouched(dg_whole)
    assert not bool((dg == SENTINEL).any()), "an element of dgates was not written"
    return res


def _host_outputs(res, K):
    """The four gradients as float64 arrays with the pad columns cut off (they are asserted zero)."""
    out = {}
    for k in L.OUTPUTS:
        v = res[k].double().cpu().numpy()
        if k in ("dx", "dw_ih"):
            assert not np.any(v[..., K:]), "%s: a zero pad column of x has a gradient" % k
            v = v[..., :K]
        out[k] = v
    return out


@pytest.mark.parametrize("T,B,H,K,dir_mask", CASES)
def test_gradients_against_float64_autograd(lib, T, B, H, K, dir_mask):
    x, layer, dout = L.make_case(T, B, H, K)
    xb, P = _operands(x, layer)
    _, _, tape, _ = _train_forward(lib, xb, P, dir_mask)
    res = _backward(lib, xb, P, tape, dout)
    got = _host_outputs(res, K)
    exact, S = L.yardstick(x, layer, dout, dir_mask)
    for k in L.OUTPUTS:
        e = L.relrms_or_zero(got[k], exact[k])
        print("%s (T %d, B %d, H %d, K %d, mask %d): relrms %.3e, rounding-only S %.3e, ratio %.2f"
              % (k, T, B, H, K, dir_mask, e, S[k], e / S[k] if S[k] else 0.0))
    assert L.yardstick_failures(got, exact, S) == []
    if T == 1:
        assert not bool(res["dw_hh"].any())  # exactly zero: no frame has a predecessor
    for d in (0, 1):
        if not dir_mask & (1 << d):
            assert not bool(res["dgates"][d].any()) and not bool(res["dw_ih"][d].any()) and not bool(res["db"][d].any())
    # two runs, the same bits
    res2 = _backward(lib, xb, P, tape, dout)
    for k in ("dgates",) + L.OUTPUTS:
        assert torch.equal(_bits(res[k]), _bits(res2[k])), k


@pytest.mark.parametrize("T,B,H,K,whh_zero", [(1, 17, 64, 40, False), (1, 65, 128, 64, False), (3, 17, 128, 40, True), (5, 16, 64, 64, True)])
def test_cell_backward_is_exact_without_a_recurrent_product(lib, T, B, H, K, whh_zero):
    """W_hh = 0, and separately T = 1: dgates is the cell backward of dout alone, within the float32 operation count of the formulas
    plus half a bf16 step (lstm_train_cases.cell_backward_bound, from the device's own tape)."""
    x, layer, dout = L.make_case(T, B, H, K, seed=3)
    if whh_zero:
        layer["weight_hh"][:] = 0
    xb, P = _operands(x, layer)
    _, _, tape, _ = _train_forward(lib, xb, P, 3)
    res = _backward(lib, xb, P, tape, dout, need_dx=False)
    act, _ = tape.views()
    exact, bound = L.cell_backward_bound(dout, act.double().cpu().numpy())
    err = np.abs(res["dgates"].double().cpu().numpy() - exact)
    print("cell backward (T %d, B %d, H %d, W_hh %s): max |err| / bound = %.3f, max |err| %.3e"
          % (T, B, H, "0" if whh_zero else "random", (err / np.maximum(bound, 1e-300)).max(), err.max()))
    assert np.all(err <= bound)
    if T == 1:
        assert not bool(res["dw_hh"].any())
        assert not np.any(res["dgates"][:, :, :, H:2 * H].double().cpu().numpy())  # df = dc c_{-1} f (1 - f), c_{-1} = 0


@pytest.mark.parametrize("T,B,H,K,t0,b0", [(5, 17, 64, 40, 2, 16), (3, 65, 128, 64, 0, 64), (2, 16, 64, 64, 1, 3), (5, 3, 128, 40, 4, 0)])
def test_gradient_routing(lib, T, B, H, K, t0, b0):
    x, layer, _ = L.make_case(T, B, H, K, seed=5)
    dout = np.zeros((T, B, H), np.float32)
    dout[t0, b0] = np.random.RandomState(t0 + b0).normal(0, 1, H)
    xb, P = _operands(x, layer)
    _, _, tape, _ = _train_forward(lib, xb, P, 3)
    res = _backward(lib, xb, P, tape, dout)
    assert L.routing_failures(res["dgates"].double().cpu().numpy(), res["dx"].double().cpu().numpy(), t0, b0) == []


@pytest.mark.parametrize("H", [64, 128])
def test_backward_pack_matches_the_restated_order(lib, H):
    layer = L.layer_params(H, 64, H)
    _, P = _operands(np.zeros((1, 1, 64)), layer)
    want = C.bf16_round(L.pack_bwd(layer["weight_hh"]))
    assert np.array_equal(P["whh_bwd"].double().cpu().numpy(), want)


def test_refusals(lib):
    """A null or misaligned pointer, H = 96, a short tape or workspace and dir_mask 0 return the documented code before any launch:
    every output buffer keeps its fill."""
    from mindaudio_amd import _lib

    T, B, H, Kpad = 3, 2, 64, 64
    buf = torch.full((1 << 20,), TAPE_FILL, dtype=torch.uint8, device="cuda")
    p, big = buf.data_ptr(), 1 << 20
    tape_bytes, ws_bytes = lib.ma_lstm_train_tape_bytes(T, B, H), lib.ma_lstm_bwd_workspace_bytes(B, H)
    fws = lib.ma_lstm_workspace_bytes(T, B, H, T)
    assert tape_bytes == 2 * T * 5 * B * H * 4 + 2 * T * B * H * 2 and lib.ma_lstm_train_tape_h_offset(T, B, H) == 2 * T * 5 * B * H * 4
    assert lib.ma_lstm_train_tape_bytes(T, B, 96) == _lib.MA_ERR_UNSUPPORTED and lib.ma_lstm_train_tape_bytes(0, B, H) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_lstm_bwd_workspace_bytes(B, 96) == _lib.MA_ERR_UNSUPPORTED

    def fwd(x=p, H=H, mask=3, tape=p, tb=big, ws=big):
        return lib.ma_lstm_bidir_train_bf16(x, T, B, Kpad, H, p, p, p, mask, T, p, p, None, tape, tb, p, ws, None)

    assert fwd(x=None) == _lib.MA_ERR_INVALID_ARG and fwd(tape=None) == _lib.MA_ERR_INVALID_ARG
    assert fwd(tape=p + 4) == _lib.MA_ERR_INVALID_ARG and fwd(x=p + 2) == _lib.MA_ERR_INVALID_ARG
    assert fwd(H=96) == _lib.MA_ERR_UNSUPPORTED
    assert fwd(mask=0) == _lib.MA_ERR_INVALID_ARG and fwd(mask=4) == _lib.MA_ERR_INVALID_ARG
    assert fwd(tb=tape_bytes - 1) == _lib.MA_ERR_WORKSPACE and fwd(ws=fws - 1) == _lib.MA_ERR_WORKSPACE

    def bwd(dout=p, H=H, mask=3, tape=p, tb=big, w=p, dg=p, ws=p, wb=big):
        return lib.ma_lstm_bidir_bwd_bf16(dout, T, B, H, tape, tb, w, mask, dg, ws, wb, None)

    for kw in (dict(dout=None), dict(tape=None), dict(w=None), dict(dg=None), dict(ws=None), dict(dout=p + 4), dict(dg=p + 2), dict(mask=0),
               dict(mask=4)):
        assert bwd(**kw) == _lib.MA_ERR_INVALID_ARG, kw
    assert bwd(H=96) == _lib.MA_ERR_UNSUPPORTED
    assert bwd(tb=tape_bytes - 1) == _lib.MA_ERR_WORKSPACE and bwd(wb=ws_bytes - 1) == _lib.MA_ERR_WORKSPACE
    assert lib.ma_lstm_pack_bwd_f32(None, H, p, None) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_lstm_pack_bwd_f32(p, H, p + 2, None) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_lstm_pack_bwd_f32(p, 96, p, None) == _lib.MA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == TAPE_FILL).all())  # nothing was launched
