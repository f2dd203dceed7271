"""GPU: the layer-pipelined LSTM stack (csrc/lstm_stack.hip), TasNet's encoder and decoder kernels (csrc/tasnet.hip), the model under
both schedules, Separation_Loss and the eval script against the float64 restatement of tests/tasnet_cases.py.

Bounds.  Saturated routing cases: 1e-6 absolute (saturation residues and float32 roundings of c over a handful of steps).
Random-weight cases: relrms(device, exact) <= 2 S with S = relrms(rounding-only, exact) computed here, per case; each test prints its
ratio relrms / S.  The encoder and decoder kernels are float32 and have element-wise bounds, derived at their tests."""
import ctypes
import re

import numpy as np
import pytest
import torch

import tasnet_cases as C

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # float32 unit roundoff
SCHEDULES = ["pipelined", "layered"]
# (T, B, H, K, layers): T < layers twice; one layer; four layers at small B; a second batch tile (B > 16: the tile kernel); a second
# workgroup row (B > 64); the yaml geometry (32 k-steps per layer: the 8-k-step blocks); 16 k-steps per layer at small B (the
# 4-k-step blocks)
STACK_TABLE = [(1, 1, 64, 64, 4), (2, 2, 64, 40, 4), (3, 1, 128, 64, 1), (19, 3, 64, 40, 4), (7, 17, 128, 160, 3), (5, 70, 256, 64, 2),
               (12, 1, 512, 500, 4), (5, 2, 256, 256, 2)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    return _lib.load()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run_stack(lib, x, layers, schedule="pipelined"):
    """x (T, B, K) float, layers: float32 parameters per layer -> (out_f32, out_bf16 as float32, h_final, c_final) NumPy arrays."""
    from mindaudio_amd import _lib

    dev = torch.device("cuda")
    T, B, K = x.shape
    H, n = layers[0]["weight_hh"].shape[1], len(layers)
    Kpad = (K + 63) // 64 * 64
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xb = torch.zeros((T, B, Kpad), dtype=torch.bfloat16, device=dev)
    xb[:, :, :K] = _dev(x).to(torch.bfloat16)
    out = torch.full((T, B, H), float("nan"), dtype=torch.float32, device=dev)
    out_bf = torch.zeros((T, B, H), dtype=torch.bfloat16, device=dev)
    hN = torch.full((n, B, H), float("nan"), dtype=torch.float32, device=dev)
    cN = torch.full((n, B, H), float("nan"), dtype=torch.float32, device=dev)
    if schedule == "pipelined":
        keep = []
        for l, p in enumerate(layers):
            Kl, Kp = (K, Kpad) if l == 0 else (H, H)
            src = [_dev(p[k]) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            packed = torch.empty((4 * H * (Kp + H),), dtype=torch.bfloat16, device=dev)
            bias = torch.empty((4 * H,), dtype=torch.float32, device=dev)
            _lib.check(lib.ma_lstm_stack_pack_f32(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), src[3].data_ptr(), Kl, Kp, H,
                                                  packed.data_ptr(), bias.data_ptr(), s), "stack_pack")
            keep.append((packed, bias, src))
        nbytes = lib.ma_lstm_stack_workspace_bytes(T, B, H, n)
        assert nbytes > 0
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        packed_ptrs = (ctypes.c_void_p * n)(*[k[0].data_ptr() for k in keep])
        bias_ptrs = (ctypes.c_void_p * n)(*[k[1].data_ptr() for k in keep])
        _lib.check(lib.ma_lstm_stack_bf16(xb.data_ptr(), T, B, Kpad, H, n, packed_ptrs, bias_ptrs, out.data_ptr(), out_bf.data_ptr(),
                                          hN.data_ptr(), cN.data_ptr(), ws.data_ptr(), nbytes, s), "lstm_stack")
    else:  # the existing layer call, forward direction only, one call per layer
        nbytes = lib.ma_lstm_workspace_bytes(T, B, H, T)
        assert nbytes > 0
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        cur = xb
        for l, p in enumerate(layers):
            Kl, Kp = (K, Kpad) if l == 0 else (H, H)
            two = [_dev(np.stack([p[k], np.zeros_like(p[k])])) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            wih = torch.empty((2, 4 * H, Kp), dtype=torch.bfloat16, device=dev)
            whh = torch.empty((2 * 4 * H * H,), dtype=torch.bfloat16, device=dev)
            bias = torch.empty((2, 4 * H), dtype=torch.float32, device=dev)
            _lib.check(lib.ma_lstm_pack_f32(two[0].data_ptr(), two[1].data_ptr(), two[2].data_ptr(), two[3].data_ptr(), Kl, Kp, H,
                                            wih.data_ptr(), whh.data_ptr(), bias.data_ptr(), s), "pack")
            o = torch.full((T, B, H), float("nan"), dtype=torch.float32, device=dev)
            ob = torch.zeros((T, B, H), dtype=torch.bfloat16, device=dev)
            c2 = torch.full((2, B, H), float("nan"), dtype=torch.float32, device=dev)
            _lib.check(lib.ma_lstm_bidir_bf16(cur.data_ptr(), T, B, Kp, H, wih.data_ptr(), whh.data_ptr(), bias.data_ptr(), 1, T,
                                              o.data_ptr(), ob.data_ptr(), c2.data_ptr(), ws.data_ptr(), nbytes, s), "lstm_layer")
            torch.cuda.synchronize()
            hN[l], cN[l] = o[T - 1], c2[0]
            cur, out, out_bf = ob, o, ob
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_bf.float().cpu().numpy(), hN.cpu().numpy(), cN.cpu().numpy()


# ---- the stack against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("T,B,H,K,layers", STACK_TABLE)
def test_stack_vs_float64(lib, T, B, H, K, layers, schedule):
    x, p, exact, rounded = C.stack_case(T, B, H, K, layers)
    got = run_stack(lib, x, p, schedule)
    for what, g, e, r in (("out", got[0], exact[0], rounded[0]), ("h_final", got[2], exact[1], rounded[1]),
                          ("c_final", got[3], exact[2], rounded[2])):
        S, err = C.relrms(r, e), C.relrms(g, e)
        print("stack %s %s (T %d, B %d, H %d, K %d, %d layers): relrms %.3e, rounding-only %.3e, ratio %.2f"
              % (schedule, what, T, B, H, K, layers, err, S, err / S))
        assert (1e-4 if what == "out" else 0) < S < 3e-2  # (the issue's condition is on the output's yardstick)
        assert err <= 2 * S


# ---- saturated routing through the stack ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("T,layers", [(1, 4), (4, 4), (7, 3)])
def test_stack_routing_saturated(lib, T, layers, H, schedule):
    x, p = C.stack_routing_case(T, 3, H, layers)
    want, want_h, want_c = C.lstm_stack(x, p)
    got, got_bf, got_h, got_c = run_stack(lib, x, p, schedule)
    err, err_h, err_c = np.abs(got - want).max(), np.abs(got_h - want_h).max(), np.abs(got_c - want_c).max()
    print("routing %s (T %d, %d layers, H %d): max |out - ref| = %.3g, |h_final - ref| = %.3g, |c_final - ref| = %.3g"
          % (schedule, T, layers, H, err, err_h, err_c))
    assert err <= 1e-6 and err_h <= 1e-6
    assert np.array_equal(got_bf, C.bf16_round(got).astype(np.float32))


# ---- invariants -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_stack_repeats_bit_for_bit_and_rows_are_independent(lib, schedule):
    p = C.stack_params(7, 40, 128, 3)
    x = np.random.RandomState(9).normal(0, 1, (6, 3, 40))
    a, b = run_stack(lib, x, p, schedule), run_stack(lib, x, p, schedule)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.array_equal(a[1], C.bf16_round(a[0]).astype(np.float32))  # out_bf16 is the rounding of out_f32
    alone = run_stack(lib, x[:, :1], p, schedule)
    assert np.array_equal(a[0][:, :1], alone[0]) and np.array_equal(a[2][:, :1], alone[2]) and np.array_equal(a[3][:, :1], alone[3])
    assert np.array_equal(a[2][-1], a[0][-1])  # h_final of the last layer is the last output frame


def test_stack_schedules_agree_to_rounding(lib):
    """The two schedules round at the same points but sum in different orders (the layered one adds a separately rounded float32
    projection): they agree to well within the yardstick, not to the bit."""
    x, p, exact, rounded = C.stack_case(19, 3, 64, 40, 4)
    a, b = run_stack(lib, x, p, "pipelined")[0], run_stack(lib, x, p, "layered")[0]
    assert C.relrms(a, b) <= 2 * C.relrms(rounded[0], exact[0])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_stack_cell_state_is_float32(lib, schedule):
    """T = 64, forget and input gates saturated open by a bias of 40, g saturated to +1, zero weights: c of layer 0 grows by exactly 1
    per step (up to 64 x 1e-14 of tanh(40) and 64 x e^-40 of the sigmoids) and ends at 64, which a bf16 c would leave at 2^8 spacing
    long before."""
    T, B, H, K = 64, 2, 64, 64
    p = [dict(weight_ih=np.zeros((4 * H, K if l == 0 else H), np.float32), weight_hh=np.zeros((4 * H, H), np.float32),
              bias_ih=np.full((4 * H,), 40.0, np.float32), bias_hh=np.zeros((4 * H,), np.float32)) for l in range(2)]
    x = np.zeros((T, B, K), np.float32)
    want, want_h, want_c = C.lstm_stack(x, p)
    assert np.abs(want_c - 64.0).max() <= 1e-9
    got, _, got_h, got_c = run_stack(lib, x, p, schedule)
    assert np.abs(got_c[0] - 64.0).max() <= 1e-5 and np.abs(got_c - want_c).max() <= 1e-5
    assert np.abs(got - want).max() <= 1e-5


# ---- ABI refusals -----------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals(lib):
    from mindaudio_amd import _lib

    assert lib.ma_lstm_stack_workspace_bytes(4, 2, 96, 2) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_lstm_stack_workspace_bytes(4, 2, 64, 9) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_lstm_stack_workspace_bytes(4, 2, 64, 0) == _lib.MA_ERR_INVALID_ARG
    buf = torch.zeros((1 << 20,), dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ptrs = (ctypes.c_void_p * 9)(*([p] * 9))

    def call(H, Kpad, n, ws):
        return lib.ma_lstm_stack_bf16(p, 4, 2, Kpad, H, n, ptrs, ptrs, p, p, None, None, p, ws, None)

    assert call(96, 64, 2, 1 << 20) == _lib.MA_ERR_UNSUPPORTED
    assert call(64, 96, 2, 1 << 20) == _lib.MA_ERR_UNSUPPORTED
    assert call(64, 64, 9, 1 << 20) == _lib.MA_ERR_UNSUPPORTED
    assert call(64, 64, 2, 16) == _lib.MA_ERR_WORKSPACE
    assert lib.ma_lstm_stack_bf16(None, 4, 2, 64, 64, 2, ptrs, ptrs, p, p, None, None, p, 1 << 20, None) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_lstm_stack_pack_f32(p, p, p, p, 64, 64, 96, p, p, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_lstm_stack_pack_f32(p, p, p, p, 64, 96, 64, p, p, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_tasnet_gated_encode_f32(p, 1, 1, 65, 40, p, p, p, p, p, p, 1e-7, p, p, p, 64, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_tasnet_gated_encode_f32(p, 1, 1, 8, 1025, p, p, p, p, p, p, 1e-7, p, p, p, 1088, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_tasnet_mask_decode_f32(p, 200, p, p, 1, 1, 5, 40, p, p, 8, p, None) == _lib.MA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched on a refusal


# ---- encoder ----------------------------------------------------------------------------------------------------------------------------------
def _model(cfg, state, schedule="pipelined"):
    from mindaudio_amd.models import TasNet

    m = TasNet(cfg["L"], cfg["N"], cfg["H"], cfg["layers"], nspk=cfg["nspk"], schedule=schedule)
    m.load_weights(state)
    return m.cuda().eval()


@pytest.mark.parametrize("B,K", [(1, 1), (3, 19)])
@pytest.mark.parametrize("N", [40, 500])
@pytest.mark.parametrize("L", [8, 40])
def test_encoder_vs_float64(lib, L, N, B, K):
    cfg = dict(L=L, N=N, H=64, layers=1, nspk=2, B=B, K=K)
    state = C.make_state(cfg, 30 + L + N)
    x = C.make_mixture(cfg, 31 + B, zero_last=B * K > 1)
    model = _model(cfg, state)
    mw, coef, xin = model.encode(x)
    torch.cuda.synchronize()
    mw, coef, xin = mw.cpu().numpy().astype(np.float64), coef.cpu().numpy().astype(np.float64), xin.float().cpu().numpy().astype(np.float64)
    w, norm, ln = C.encoder(state, x)
    f = lambda k: np.abs(np.asarray(state[k], np.float64))  # noqa: E731

    # norm_coef: a float32 sum of L squares (each rounding at most U of a partial sum <= the total: (L + 1) U relative), halved by the
    # square root, which adds its own rounding
    assert np.all(np.abs(coef - norm) <= (0.5 * (L + 1) + 2) * U * norm)
    # xn = x / (norm + 1e-8): the norm's error, the addition and the division: dx relative
    dx = (0.5 * (L + 1) + 5) * U
    xn = np.abs(x.astype(np.float64)) / (norm[..., None] + C.EPS)
    # pre-activations: an fmaf chain of L terms started at the bias, |error| <= ((L + 1) U + dx) * (sum |xn w| + |b|)
    Eu = ((L + 1) * U + dx) * (xn @ f("encoder.conv1d_U.weight")[:, :, 0].T + f("encoder.conv1d_U.bias"))
    Ev = ((L + 1) * U + dx) * (xn @ f("encoder.conv1d_V.weight")[:, :, 0].T + f("encoder.conv1d_V.bias"))
    xs = x.astype(np.float64) / (norm[..., None] + C.EPS)
    relu = np.maximum(xs @ np.asarray(state["encoder.conv1d_U.weight"], np.float64)[:, :, 0].T + np.asarray(state["encoder.conv1d_U.bias"], np.float64), 0)
    sig = C.sigmoid(xs @ np.asarray(state["encoder.conv1d_V.weight"], np.float64)[:, :, 0].T + np.asarray(state["encoder.conv1d_V.bias"], np.float64))
    # relu is 1-Lipschitz, sigmoid 1/4-Lipschitz; expf, the addition and the division of the sigmoid: 8 U relative; the product: 2 U
    bw = (relu + Eu) * (Ev / 4 + 8 * U * sig) + sig * Eu + 2 * U * w
    excess = (np.abs(mw - w) - bw).max()
    print("encoder L %d N %d B %d K %d: max |mixture_w err| %.3e, max (|err| - bound) %.3e" % (L, N, B, K, np.abs(mw - w).max(), excess))
    assert excess <= 0

    # LayerNorm, stored as bf16: |err| <= 2^-8 |y| (the store: half an ulp of 8 significant bits) + the float32 term.  With e the
    # largest error of a w plus that of the float32 mean (N U max |w|), d = w - mean is off by at most 2 e, sigma = sqrt(mean d^2 +
    # eps) by at most 2 e + N U sigma, z = d / sigma by 2 e / sigma + |z| (that, relative) + 3 U |z|, and y = z gamma + beta adds
    # 2 U (|y| + |beta|).
    got = xin.reshape(K, B, -1).transpose(1, 0, 2)
    assert got.shape[2] == (N + 63) // 64 * 64 and not got[:, :, N:].any()  # the pad columns stay zero
    got = got[:, :, :N]
    mean = w.mean(2, keepdims=True)
    sigma = np.sqrt(((w - mean) ** 2).mean(2, keepdims=True) + C.LN_EPS)
    z = (w - mean) / sigma
    e = bw.max(2, keepdims=True) + N * U * np.abs(w).max(2, keepdims=True)
    dz = 2 * e / sigma + np.abs(z) * ((2 * e + N * U * sigma) / sigma) + 3 * U * np.abs(z)
    bound = 2.0 ** -8 * np.abs(ln) + f("separator.layer_norm.gamma") * dz + 2 * U * (np.abs(ln) + f("separator.layer_norm.beta"))
    excess = (np.abs(got - ln) - bound).max()
    print("encoder L %d N %d B %d K %d: max |layer norm err| %.3e, max (|err| - bound) %.3e" % (L, N, B, K, np.abs(got - ln).max(), excess))
    assert excess <= 0
    assert np.isfinite(mw).all() and np.isfinite(got).all()
    if B * K > 1:  # the all-zero segment
        assert coef[-1, -1] == 0.0 and norm[-1, -1] == 0.0 and np.abs(got[-1, -1]).max() > 0.1


# ---- mask + decode ----------------------------------------------------------------------------------------------------------------------------
def _decode(lib, score, mw, coef, basis, bias, nspk):
    from mindaudio_amd import _lib

    B, K, N = mw.shape
    L = basis.shape[0]
    ld = (nspk * N + 7) // 8 * 8
    sc = torch.full((K * B, ld), float("nan"), dtype=torch.float32, device="cuda")
    sc[:, :nspk * N] = _dev(score.transpose(1, 0, 2).reshape(K * B, nspk * N))  # row k * B + b, as the fc GEMM leaves it
    out = torch.full((B, nspk, K, L), float("nan"), dtype=torch.float32, device="cuda")
    t = [_dev(a) for a in (mw, coef, basis, bias)]
    _lib.check(lib.ma_tasnet_mask_decode_f32(sc.data_ptr(), ld, t[0].data_ptr(), t[1].data_ptr(), B, K, nspk, N, t[2].data_ptr(),
                                             t[3].data_ptr(), L, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mask_decode")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("L,N", [(8, 40), (40, 500)])
@pytest.mark.parametrize("nspk", [2, 3])
def test_mask_decode(lib, nspk, L, N):
    g = np.random.RandomState(nspk * 100 + N)
    B, K = 2, 3
    mw = np.abs(g.normal(0, 1, (B, K, N))).astype(np.float32)
    coef = np.abs(g.normal(1, 0.3, (B, K))).astype(np.float32)
    coef[1, 2] = 0.0  # an all-zero segment
    basis = g.uniform(-0.3, 0.3, (L, N)).astype(np.float32)
    bias = g.uniform(-0.1, 0.1, (L,)).astype(np.float32)
    p = {"decoder.basis_signals.weight": basis, "decoder.basis_signals.bias": bias}
    ab, abias = np.abs(basis.astype(np.float64)), np.abs(bias.astype(np.float64))

    def bound(mask_terms):
        # a float32 dot of length N in any order: each of its N roundings is at most U of a partial sum <= sum |terms|; the bias add
        # and the multiplication by norm_coef: 2 more; `mask_terms`: the relative error of a source_w term before it enters the sum
        t = np.einsum("bksn,ln->bksl", mw.astype(np.float64)[:, :, None, :] * np.ones((1, 1, nspk, 1)), ab) + abias
        return ((N + 2 + mask_terms) * U * t * coef.astype(np.float64)[:, :, None, None]).transpose(0, 2, 1, 3)

    # prescribed scores: n even -> speaker n % nspk alone (the others 300 below: expf underflows to 0, the mask is exactly one-hot);
    # n odd -> speakers 0 and 1 tie and any third is 203.5 below: exactly one half each.  source_w is then exact in float32.
    score = np.full((B, K, nspk, N), -200.0, np.float32)
    want_mask = np.zeros((nspk, N))
    for n in range(N):
        if n % 2 == 0:
            score[:, :, n % nspk, n] = 100.0
            want_mask[n % nspk, n] = 1.0
        else:
            score[:, :, :2, n] = 3.5
            want_mask[:2, n] = 0.5
    got = _decode(lib, score.reshape(B, K, nspk * N), mw, coef, basis, bias, nspk)
    sw = mw.astype(np.float64)[:, :, None, :] * want_mask
    want = ((sw @ basis.astype(np.float64).T + bias) * coef.astype(np.float64)[:, :, None, None]).transpose(0, 2, 1, 3)
    assert got.shape == (B, nspk, K, L)
    assert np.abs(want - C.mask_decode(p, score.reshape(B, K, nspk * N), mw, coef, nspk)).max() <= 1e-12
    excess = (np.abs(got - want) - bound(0)).max()
    print("mask_decode prescribed nspk %d L %d N %d: max |err| %.3e, max (|err| - bound) %.3e" % (nspk, L, N, np.abs(got - want).max(), excess))
    assert excess <= 0
    assert np.all(got[1, :, 2, :] == 0.0) and np.abs(got[0]).max() > 0  # norm_coef = 0 multiplies the bias too: exactly zero

    # random scores against float64: the softmax (expf, nspk - 1 additions, a division, the product with mixture_w) is good to
    # (8 + nspk) U relative per term
    score = g.normal(0, 3, (B, K, nspk * N)).astype(np.float32)
    got = _decode(lib, score, mw, coef, basis, bias, nspk)
    want = C.mask_decode(p, score, mw, coef, nspk)
    excess = (np.abs(got - want) - bound(8 + nspk)).max()
    print("mask_decode random nspk %d L %d N %d: max |err| %.3e, max (|err| - bound) %.3e" % (nspk, L, N, np.abs(got - want).max(), excess))
    assert excess <= 0


# ---- model ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ["small", "yaml-geometry"])
def test_model_vs_float64(lib, name, schedule):
    cfg, state, x, exact, rounded, h, hr = C.model_case(name)
    S = C.relrms(rounded, exact)
    model = _model(cfg, state, schedule)
    est = model(x)  # NumPy in
    assert tuple(est.shape) == exact.shape == (cfg["B"], cfg["nspk"], cfg["K"], cfg["L"]) and est.dtype == torch.float32 and est.is_cuda
    got = est.cpu().numpy()
    e = C.relrms(got, exact)
    print("model %s %s: relrms %.3e, rounding-only %.3e, ratio %.2f" % (name, schedule, e, S, e / S))
    assert 1e-4 < S < 3e-2 and e <= 2 * S
    assert not got[-1, :, -1].any()  # the all-zero last segment
    assert np.array_equal(model(torch.from_numpy(x).cuda()).cpu().numpy(), got)  # a device tensor in; the same bits
    model.schedule = "layered" if schedule == "pipelined" else "pipelined"
    assert C.relrms(model(x).cpu().numpy(), exact) <= 2 * S  # the other schedule on the same prepared weights
    model.schedule = schedule
    if name == "small":
        # the stale-weights trap: weights loaded after a forward must be used
        state2 = C.make_state(cfg, 99)
        model.load_weights(state2)
        got2 = model(x).cpu().numpy()
        exact2 = C.forward(state2, cfg, x)[0]
        assert C.relrms(got2, exact2) <= 2 * C.relrms(C.forward(state2, cfg, x, rounding=True)[0], exact2)
        assert C.relrms(got2, exact) > 0.5


def test_model_refuses_bidirectional(lib):
    from mindaudio_amd.models import TasNet

    with pytest.raises(NotImplementedError, match="reference cannot run it either"):
        TasNet(40, 500, 512, 4, bidirectional=True)


# ---- Separation_Loss --------------------------------------------------------------------------------------------------------------------------
def test_separation_loss_vs_restatement(lib):
    from mindaudio_amd.loss import Separation_Loss

    g = np.random.RandomState(5)
    B, K, L = 3, 11, 8
    source = (g.normal(0, 1, (B, 2, K, L)) + 0.2).astype(np.float32)
    estimate = (source + 0.3 * g.normal(0, 1, source.shape)).astype(np.float32)
    estimate[1] = estimate[1, ::-1]
    for lengths in ([K, K, K], [K, 5, 7]):
        want = C.separation_loss(source, estimate, lengths)
        est = torch.from_numpy(estimate).cuda()
        loss, max_snr, same, reordered = Separation_Loss()(torch.from_numpy(source).cuda(), est, torch.tensor(lengths))
        assert same is est and tuple(max_snr.shape) == (B, 1) and tuple(reordered.shape) == (B, 2, K, L)
        # float64 arithmetic on float32 data; max_snr and the loss are returned in float32: 2^-24 relative of values up to ~20 dB
        assert np.abs(max_snr.cpu().numpy() - want[1]).max() <= 1e-5 and abs(float(loss) - want[0]) <= 1e-5
        assert np.array_equal(reordered.cpu().numpy(), want[3].astype(np.float32))
        assert want[2].tolist() == [[0, 1], [1, 0], [0, 1]]


# ---- eval end to end ----------------------------------------------------------------------------------------------------------------------------
def _lines_values(lines):
    vals = [float(m.group(1)) for l in lines for m in [re.fullmatch(r"\tSI-SNRi=(-?\d+\.\d\d)", l)] if m]
    avg = [float(m.group(1)) for l in lines for m in [re.fullmatch(r"Average SISNR improvement: (-?\d+\.\d\d)", l)] if m]
    return vals, avg


def test_eval_prescribed_model(lib, tmp_path):
    """Estimates = the sources swapped, plus small noise: the loss must swap them back, and every printed figure is computed here."""
    from mindaudio_amd.metric import cal_SISNRi
    from mindaudio_amd.tasnet.eval import evaluate

    waves = C.write_dataset(str(tmp_path), [900, 1300, 1100], ["b", "a", "c"])
    noise = (0.001 * np.random.RandomState(2).normal(0, 1, (3, 2, 3320, 40))).astype(np.float32)
    order = ["a", "c", "b"]  # (#samples, path) descending
    pad = lambda w: np.concatenate([w, np.zeros(132800 - len(w), np.float32)])  # noqa: E731
    sources = np.stack([np.stack([pad(waves[n][1]), pad(waves[n][2])]) for n in order]).reshape(3, 2, 3320, 40)
    seen = []

    def model(mixture):
        assert mixture.is_cuda and mixture.dtype == torch.float32 and tuple(mixture.shape[1:]) == (3320, 40)
        first = sum(seen)
        seen.append(mixture.shape[0])
        return torch.from_numpy(sources[first:first + mixture.shape[0], ::-1].copy() + noise[first:first + mixture.shape[0]]).cuda()

    lines = []
    config = dict(data_dir=str(tmp_path), eval_batch_size=2, sample_rate=8000, L=40, cal_sdr=0)
    average, values = evaluate(config, model=model, log=lambda *a: lines.append(" ".join(str(v) for v in a)))
    assert seen == [2, 1]
    want = [float(cal_SISNRi(sources[i].reshape(2, -1), (sources[i] + noise[i, ::-1]).reshape(2, -1), pad(waves[n][0])))
            for i, n in enumerate(order)]
    assert np.abs(np.array(values) - np.array(want)).max() <= 1e-9 and min(want) > 10
    expect = []
    for i, v in enumerate(want):
        expect += ["Utt %d" % (i + 1), "\tSI-SNRi={0:.2f}".format(v)]
    assert lines == expect + ["Average SISNR improvement: {0:.2f}".format(sum(want) / 3)]
    assert average == sum(values) / 3
    with pytest.raises(NotImplementedError, match="mir_eval"):
        evaluate(dict(config, cal_sdr=1), model=model)


def test_eval_real_small_model(lib, tmp_path, capsys):
    """A real model from a written checkpoint through the command line's entry point; the printed average is the mean of cal_SISNRi
    over the model's own outputs, reordered by the float64 restatement of the loss."""
    import yaml

    from mindaudio_amd.metric import cal_SISNRi
    from mindaudio_amd.tasnet import DatasetGenerator
    from mindaudio_amd.tasnet import eval as tasnet_eval
    from mindaudio_amd.utils import ckpt

    C.write_dataset(str(tmp_path), [700, 1200, 1000], ["x", "y", "z"], seed=1)
    cfg = dict(L=40, N=40, H=64, layers=2, nspk=2)
    state = C.make_state(cfg, 8)
    path = str(tmp_path / "small.ckpt")
    ckpt.write_mindspore_ckpt(path, ckpt.tasnet_to_reference_names(state))
    config = dict(data_dir=str(tmp_path), eval_batch_size=2, sample_rate=8000, nspk=2, L=40, N=40, bidirectional=0, hidden_size=64,
                  num_layers=2, model_path=path, cal_sdr=0)
    ypath = str(tmp_path / "tasnet.yaml")
    with open(ypath, "w") as fh:
        yaml.safe_dump(config, fh)
    average, values = tasnet_eval.main(["--config_path", ypath])
    lines = capsys.readouterr().out.split("\n")
    printed, avg = _lines_values(lines)
    assert sum(l.startswith("Utt ") for l in lines) == 3 and len(printed) == 3 and len(avg) == 1
    assert lines[0] == "=====> load params into generator"

    model = _model(cfg, state)
    ds = DatasetGenerator(str(tmp_path), 2, L=40)
    want = []
    for first in (0, 2):
        items = [ds[i] for i in range(first, min(first + 2, 3))]
        mix, src = np.stack([it[0] for it in items]), np.stack([it[2] for it in items])
        est = model(mix).cpu().numpy()
        reordered = C.separation_loss(src, est, [3320] * len(items))[3]
        want += [float(cal_SISNRi(src[i].reshape(2, -1), reordered[i].reshape(2, -1), mix[i].reshape(-1))) for i in range(len(items))]
    assert np.abs(np.array(values) - np.array(want)).max() <= 1e-6  # (the same bits from the model; the metric is float64)
    assert abs(avg[0] - sum(want) / 3) <= 5e-3 + 1e-6 and all(abs(a - b) <= 5e-3 + 1e-6 for a, b in zip(printed, want))
    assert average == sum(values) / 3
