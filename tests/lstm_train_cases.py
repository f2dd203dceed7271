"""The float64 restatement of ONE bidirectional LSTM layer's training step that test_lstm_train_cases_cpu.py and test_lstm_train_gpu.py
measure against (csrc/lstm.hip's training forward, csrc/lstm_train.hip's backward through time, and the products that follow it).

  layer_step       the forward and the CLOSED-FORM backward, in two modes: `rounding=True` rounds to bf16 exactly where the device does -
                   x, W_ih, W_hh, the h that is fed back (the tape's h image) and dgates (the stored result, which is also the next
                   step's operand and the operand of the dW / dx products) - `rounding=False` rounds nothing.
  autograd_step    the same layer as a torch.autograd float64 graph: the independent yardstick, nothing rounded.
  DEFECTS          planted mistakes of layer_step's backward; the CPU tests show that the comparators below reject each of them.
  comparators      yardstick_failures (2 S, the project's convention), routing_failures (exact zeros), cell_backward_bound (pointwise).

Layouts: x (T, B, K); layer = {weight_ih (2, 4H, K), weight_hh (2, 4H, H), bias_ih, bias_hh (2, 4H)}, directions stacked forward /
reverse, gate order i, f, g, o; act (2, T, 5, B, H) = the ACTIVATED gates i, f, g, o and c_t; h (2, T, B, H); dgates (2, T, B, 4H).
No figure in this file is measured on the code under test."""
import numpy as np
import torch

from deepspeech2_cases import bf16_round, relrms, sigmoid

U = 2.0 ** -24          # half an ulp of a float32 value, relative: the rounding of one float32 operation
BF16_HALF = 2.0 ** -8   # half a bf16 step, relative (8 significant bits)
TANH_ULP = 5            # tanhf within 5 ulp: the OpenCL / HIP device-library requirement for tanh (the measured error is smaller)

DEFECTS = ("c_prev_first", "reverse_as_forward", "dout_one_dir", "h_shift", "gate_order", "no_dc_carry", "db_one_dir")
OUTPUTS = ("dx", "dw_ih", "dw_hh", "db")


# ---- forward with a tape ------------------------------------------------------------------------------------------------------------------
def _direction_forward(x, w_ih, w_hh, bias, reverse, r):
    T, B, _ = x.shape
    H = w_hh.shape[1]
    act, hfed, out = np.zeros((T, 5, B, H)), np.zeros((T, B, H)), np.zeros((T, B, H))
    h, c = np.zeros((B, H)), np.zeros((B, H))
    for s in range(T):
        t = T - 1 - s if reverse else s
        gates = x[t] @ w_ih.T + bias + h @ w_hh.T
        i, f, g, o = sigmoid(gates[:, :H]), sigmoid(gates[:, H:2 * H]), np.tanh(gates[:, 2 * H:3 * H]), sigmoid(gates[:, 3 * H:])
        c = f * c + i * g
        out[t] = o * np.tanh(c)
        h = r(out[t])  # what is fed back (and kept on the tape)
        act[t], hfed[t] = np.stack([i, f, g, o, c]), h
    return act, hfed, out


# ---- the cell backward, closed form ---------------------------------------------------------------------------------------------------------
def cell_backward(dh, dc_next, i, f, g, o, c, c_prev):
    """-> (di, df, dg, do, dc_next for the step before): include/mindaudio_amd.h's formulas."""
    th = np.tanh(c)
    dc = dh * o * (1 - th * th) + dc_next
    return dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * th * o * (1 - o), dc * f


def _direction_backward(dout, act, hfed, w_hh, reverse, r, defect):
    """-> (dgates (T, B, 4H), the frame before each t in the direction's forward walk, or -1)"""
    T, _, B, H = act.shape
    walk_reverse = reverse and defect != "reverse_as_forward"
    order = range(T) if walk_reverse else range(T - 1, -1, -1)
    dgates, before = np.zeros((T, B, 4 * H)), np.zeros(T, int)
    dc_next, dg_next = np.zeros((B, H)), None
    for t in order:
        p = t + 1 if walk_reverse else t - 1
        before[t] = p if 0 <= p < T else -1
        i, f, g, o, c = act[t]
        c_prev = act[p, 4] if before[t] >= 0 else (c if defect == "c_prev_first" else np.zeros((B, H)))
        dh = dout[t] + (dg_next @ w_hh if dg_next is not None else 0.0)
        di, df, dg, do, dcf = cell_backward(dh, dc_next, i, f, g, o, c, c_prev)
        parts = [di, dg, df, do] if defect == "gate_order" else [di, df, dg, do]
        dg_next = dgates[t] = r(np.concatenate(parts, axis=1))
        dc_next = np.zeros((B, H)) if defect == "no_dc_carry" else dcf
    return dgates, before


def layer_step(x, layer, dout, rounding=False, dir_mask=3, defect=None):
    """-> {out (T, B, H), act, h, dgates, dx (T, B, K), dw_ih (2, 4H, K), dw_hh (2, 4H, H), db (2, 4H)}; a direction outside dir_mask
    contributes nothing and has zero gradients."""
    assert defect is None or defect in DEFECTS
    r = bf16_round if rounding else (lambda a: np.asarray(a, np.float64))
    x = r(np.asarray(x, np.float64))
    T, B, K = x.shape
    H = layer["weight_hh"].shape[2]
    dout = np.asarray(dout, np.float64)
    res = dict(out=np.zeros((T, B, H)), act=np.zeros((2, T, 5, B, H)), h=np.zeros((2, T, B, H)), dgates=np.zeros((2, T, B, 4 * H)),
               dx=np.zeros((T, B, K)), dw_ih=np.zeros((2, 4 * H, K)), dw_hh=np.zeros((2, 4 * H, H)), db=np.zeros((2, 4 * H)))
    for d in (0, 1):
        if not dir_mask & (1 << d):
            continue
        w_ih, w_hh = r(np.asarray(layer["weight_ih"][d], np.float64)), r(np.asarray(layer["weight_hh"][d], np.float64))
        bias = np.asarray(layer["bias_ih"][d], np.float64) + np.asarray(layer["bias_hh"][d], np.float64)
        act, hfed, out = _direction_forward(x, w_ih, w_hh, bias, d == 1, r)
        dd = np.zeros_like(dout) if (defect == "dout_one_dir" and d == 1) else dout
        dg, before = _direction_backward(dd, act, hfed, w_hh, d == 1, r, defect)
        res["out"] += out
        res["act"][d], res["h"][d], res["dgates"][d] = act, hfed, dg
        res["dx"] += dg @ w_ih
        res["dw_ih"][d] = dg.reshape(T * B, -1).T @ x.reshape(T * B, K)
        res["db"][d] = dg.sum((0, 1))
        for t in range(T):
            src = t if defect == "h_shift" else before[t]
            if src >= 0:
                res["dw_hh"][d] += dg[t].T @ hfed[src]
    if defect == "db_one_dir":
        res["db"][1] = 0.0
    return res


# ---- the independent yardstick --------------------------------------------------------------------------------------------------------------
def autograd_step(x, layer, dout, dir_mask=3):
    """The layer as a float64 torch graph (nothing rounded), differentiated by torch.autograd -> {out, dx, dw_ih, dw_hh, db_ih, db_hh}."""
    f64 = torch.float64
    xt = torch.tensor(np.asarray(x, np.float64), dtype=f64, requires_grad=True)
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=f64, requires_grad=True) for k, v in layer.items()}
    T, B, _ = xt.shape
    H = p["weight_hh"].shape[2]
    out = [torch.zeros((B, H), dtype=f64) for _ in range(T)]
    for d in (0, 1):
        if not dir_mask & (1 << d):
            continue
        h, c = torch.zeros((B, H), dtype=f64), torch.zeros((B, H), dtype=f64)
        for s in range(T):
            t = T - 1 - s if d == 1 else s
            gates = xt[t] @ p["weight_ih"][d].T + p["bias_ih"][d] + h @ p["weight_hh"][d].T + p["bias_hh"][d]
            i, f, g, o = gates.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[t] = out[t] + h
    out = torch.stack(out)
    out.backward(torch.tensor(np.asarray(dout, np.float64), dtype=f64))

    def grad(t):
        return (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()

    return dict(out=out.detach().numpy(), dx=grad(xt), dw_ih=grad(p["weight_ih"]), dw_hh=grad(p["weight_hh"]), db_ih=grad(p["bias_ih"]),
                db_hh=grad(p["bias_hh"]))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def layer_params(seed, K, H, scale=1.0):
    """uniform(+- scale / sqrt(H)) float32, both directions stacked: nn.LSTM's initialisation at scale 1."""
    g = np.random.RandomState(seed)
    k = scale / np.sqrt(H)
    return {n: g.uniform(-k, k, (2,) + s).astype(np.float32) for n, s in
            (("weight_ih", (4 * H, K)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,)))}


def make_case(T, B, H, K, seed=0, w_scale=2.0):
    """(x, layer, dout): x a bf16 activation (as every producer leaves it), weights at twice nn.LSTM's scale so that the recurrent
    path carries a visible share of every gradient, dout unit normal."""
    g = np.random.RandomState(7000 + seed + 11 * T + 13 * B + H + K)
    x = bf16_round(g.normal(0, 1, (T, B, K)))
    return x, layer_params(seed + T + B, K, H, w_scale), g.normal(0, 1, (T, B, H)).astype(np.float32)


# ---- comparators ----------------------------------------------------------------------------------------------------------------------------
def yardstick(x, layer, dout, dir_mask=3):
    """-> (exact: autograd_step's outputs under OUTPUTS' names, S: {output: relrms(rounded restatement, exact)})"""
    ref = autograd_step(x, layer, dout, dir_mask)
    assert np.array_equal(ref["db_ih"], ref["db_hh"])
    exact = dict(dx=ref["dx"], dw_ih=ref["dw_ih"], dw_hh=ref["dw_hh"], db=ref["db_ih"])
    rounded = layer_step(x, layer, dout, rounding=True, dir_mask=dir_mask)
    return exact, {k: relrms_or_zero(rounded[k], exact[k]) for k in OUTPUTS}


def relrms_or_zero(got, ref):
    if not np.any(ref):  # an output that is exactly zero (dw_hh at T = 1) has no relative error: it must be zero
        return 0.0 if not np.any(got) else float("inf")
    return relrms(got, ref)


def yardstick_failures(got, exact, S, factor=2.0):
    """The outputs whose relative rms error against the unrounded float64 autograd exceeds factor * S (2: the project's convention for
    what float32 accumulation order and float32 sigmoid / tanh add to the rounding points) -> [(name, relrms, S)]."""
    bad = []
    for k in OUTPUTS:
        e = relrms_or_zero(got[k], exact[k])
        if not e <= factor * S[k]:
            bad.append((k, e, S[k]))
    return bad


def routing_failures(dgates, dx, t0, b0):
    """dout non-zero at (t0, b0) only: every dgates and dx row of another batch row is exactly zero, the forward direction has nothing
    after t0 and the reverse direction nothing before it; the rows that may be non-zero are not all zero."""
    dgates, bad = np.asarray(dgates, np.float64), []
    others = [b for b in range(dgates.shape[2]) if b != b0]
    if np.any(dgates[:, :, others]):
        bad.append("dgates: another batch row is non-zero")
    if np.any(dgates[0, t0 + 1:]):
        bad.append("dgates: the forward direction is non-zero after t0")
    if np.any(dgates[1, :t0]):
        bad.append("dgates: the reverse direction is non-zero before t0")
    if not (np.any(dgates[0, t0, b0]) and np.any(dgates[1, t0, b0])):
        bad.append("dgates: (t0, b0) itself is zero")
    if dx is not None and np.any(np.asarray(dx)[:, others]):
        bad.append("dx: another batch row is non-zero")
    return bad


def cell_backward_bound(dout, act, dir_mask=3):
    """dgates of a layer WITHOUT a recurrent product (W_hh = 0, or T = 1), where dh = dout exactly: the float64 cell backward of the
    given tape (the device's own float32 tape, so the forward's error does not enter) and an element-wise bound on what a float32
    evaluation of include/mindaudio_amd.h's formulas followed by a bf16 store may differ from it.  -> (exact, bound), (2, T, B, 4H).

    Derivation, u = 2^-24 (one float32 rounding, relative), every float32 operation counted once, FMA contraction only removes some:
      th = tanhf(c)                    relative tau = 2 * TANH_ULP u
      A = 1 - th^2                     th^2: (2 tau + u) th^2 <= 2 tau + u absolute; the subtraction u A:  |err A| <= 2 tau + 2 u
      dc = dh o A + dc_next            |dh o| |err A| + 2 u |dh o A| + u |dc| + e_next =: E     (e_next: the error carried in dc_next)
      do = dh th (o (1 - o))           four roundings and tau:  (4 u + tau) |do|
      di = dc g (i (1 - i))            4 u |di| + E |g i (1 - i)|
      dg = dc i (1 - g^2)              1 - g^2: 2 u absolute;  2 u |dc i| + 2 u |dg| + E |i (1 - g^2)|
      df = dc c_prev (f (1 - f))       4 u |df| + E |c_prev f (1 - f)|
      dc_next <- dc f                  e = E |f| + u |dc f|
      store                            half a bf16 step of the float32 value: BF16_HALF (|exact| + float32 error)"""
    act = np.asarray(act, np.float64)
    dout = np.asarray(dout, np.float64)
    _, T, _, B, H = act.shape
    tau = 2 * TANH_ULP * U
    exact, bound = np.zeros((2, T, B, 4 * H)), np.zeros((2, T, B, 4 * H))
    for d in (0, 1):
        if not dir_mask & (1 << d):
            continue
        dc_next, e_next = np.zeros((B, H)), np.zeros((B, H))
        for t in (range(T) if d == 1 else range(T - 1, -1, -1)):
            p = t + 1 if d == 1 else t - 1
            i, f, g, o, c = act[d, t]
            c_prev = act[d, p, 4] if 0 <= p < T else np.zeros((B, H))
            dh = dout[t]
            th = np.tanh(c)
            A = 1 - th * th
            dc = dh * o * A + dc_next
            E = np.abs(dh * o) * (2 * tau + 2 * U) + 2 * U * np.abs(dh * o * A) + U * np.abs(dc) + e_next
            di, df, dg, do, dcf = cell_backward(dh, dc_next, i, f, g, o, c, c_prev)
            err = [4 * U * np.abs(di) + E * np.abs(g * i * (1 - i)),
                   4 * U * np.abs(df) + E * np.abs(c_prev * f * (1 - f)),
                   2 * U * np.abs(dc * i) + 2 * U * np.abs(dg) + E * np.abs(i * (1 - g * g)),
                   (4 * U + tau) * np.abs(do)]
            exact[d, t] = np.concatenate([di, df, dg, do], axis=1)
            e32 = np.concatenate(err, axis=1)
            bound[d, t] = e32 + BF16_HALF * (np.abs(exact[d, t]) + e32)
            dc_next, e_next = dcf, E * np.abs(f) + U * np.abs(dcf)
    return exact, bound


# ---- the backward fragment order of W_hh (csrc/lstm_common.h: lstm_bwd_fragment) --------------------------------------------------------------
def bwd_fragment(i, H):
    """Fragment i (8 elements) of the backward packing of a (2, 4H, H) W_hh -> (direction, first gate row k, hidden column n): it holds
    W_hh[direction][k .. k + 7][n]."""
    nk = H // 8  # k-steps of 32 over 4H
    lane, q = i & 63, i >> 6
    unit = q // nk * 16 + (lane & 15)
    return unit // H, (q % nk) * 32 + 8 * (lane >> 4), unit % H


def pack_bwd(w_hh):
    """(2, 4H, H) -> the packed order, 2 * 4H * H values."""
    w_hh = np.asarray(w_hh)
    H = w_hh.shape[2]
    out = np.zeros(2 * 4 * H * H, w_hh.dtype)
    for i in range(out.size // 8):
        d, k, n = bwd_fragment(i, H)
        out[8 * i:8 * i + 8] = w_hh[d, k:k + 8, n]
    return out


def unpack_bwd(packed, H):
    out = np.zeros((2, 4 * H, H), np.asarray(packed).dtype)
    for i in range(np.asarray(packed).size // 8):
        d, k, n = bwd_fragment(i, H)
        out[d, k:k + 8, n] = packed[8 * i:8 * i + 8]
    return out
