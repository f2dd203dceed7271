"""CPU: the yardsticks of tests/lstm_train_cases.py themselves.  The closed-form backward equals torch.autograd in float64, every
planted defect is rejected by the comparators that test_lstm_train_gpu.py applies to the device's results, and the backward fragment
order of W_hh is a bijection."""
import numpy as np
import pytest

import lstm_train_cases as L

# (T, B, H, K, dir_mask): small relatives of the GPU shapes (the restatement's cost is T matrix products per direction)
CASES = [(1, 2, 8, 5, 3), (2, 3, 8, 5, 3), (3, 2, 16, 8, 3), (5, 3, 16, 8, 3), (5, 2, 8, 5, 1), (4, 2, 8, 5, 2)]
# the shape the defect tests run at is one of the GPU yardstick test's own (T = 5: every defect has frames to show in)
DEFECT_CASE = (5, 17, 64, 40)


@pytest.mark.parametrize("T,B,H,K,dir_mask", CASES)
def test_closed_form_equals_autograd_in_float64(T, B, H, K, dir_mask):
    x, layer, dout = L.make_case(T, B, H, K)
    mine, ref = L.layer_step(x, layer, dout, dir_mask=dir_mask), L.autograd_step(x, layer, dout, dir_mask)
    for got, want in ((mine["out"], ref["out"]), (mine["dx"], ref["dx"]), (mine["dw_ih"], ref["dw_ih"]), (mine["dw_hh"], ref["dw_hh"]),
                      (mine["db"], ref["db_ih"]), (mine["db"], ref["db_hh"])):
        # round-off of sums of up to T B K float64 products of O(1) values
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if T == 1:
        assert not np.any(mine["dw_hh"]) and not np.any(ref["dw_hh"])
    if dir_mask != 3:
        off = 0 if dir_mask == 2 else 1
        assert not np.any(mine["dw_ih"][off]) and not np.any(ref["dw_ih"][off]) and not np.any(mine["dgates"][off])


@pytest.fixture(scope="module")
def defect_case():
    T, B, H, K = DEFECT_CASE
    x, layer, dout = L.make_case(T, B, H, K)
    exact, S = L.yardstick(x, layer, dout)
    return x, layer, dout, exact, S


def test_rounded_restatement_passes_its_own_comparators(defect_case):
    x, layer, dout, exact, S = defect_case
    for k in L.OUTPUTS:
        assert 0 < S[k] < 3e-2, (k, S[k])  # bf16 rounding points: a fraction of a percent
    assert L.yardstick_failures(L.layer_step(x, layer, dout, rounding=True), exact, S) == []
    # and an unrounded float32-sized perturbation of the exact result passes as well
    assert L.yardstick_failures({k: v * (1 + 1e-6) for k, v in exact.items()}, exact, S) == []


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_planted_defect_is_rejected(defect_case, defect):
    x, layer, dout, exact, S = defect_case
    got = L.layer_step(x, layer, dout, rounding=True, defect=defect)
    bad = L.yardstick_failures(got, exact, S)
    print(defect, [(k, "%.3e vs S %.3e" % (e, s)) for k, e, s in bad])
    assert bad, "the 2 S comparator accepts the defect %r" % defect


@pytest.mark.parametrize("defect", ["reverse_as_forward", "dout_one_dir"])
def test_routing_comparator_rejects_direction_defects(defect):
    T, B, H, K, t0, b0 = 5, 3, 8, 5, 2, 1
    x, layer, _ = L.make_case(T, B, H, K)
    dout = np.zeros((T, B, H), np.float32)
    dout[t0, b0] = np.random.RandomState(3).normal(0, 1, H)
    good = L.layer_step(x, layer, dout, rounding=True)
    assert L.routing_failures(good["dgates"], good["dx"], t0, b0) == []
    bad = L.layer_step(x, layer, dout, rounding=True, defect=defect)
    assert L.routing_failures(bad["dgates"], bad["dx"], t0, b0)
    # a gradient that leaks into another batch row is caught too
    leak = good["dgates"].copy()
    leak[0, 0, 0, 3] = 1e-30
    assert L.routing_failures(leak, good["dx"], t0, b0)


@pytest.mark.parametrize("defect", ["c_prev_first", "gate_order", "no_dc_carry"])
def test_pointwise_comparator_rejects_cell_defects(defect):
    """W_hh = 0: dgates is the cell backward of dout alone; the bound holds for the correct float32-sized result and fails for the cell
    defects (T = 3, so that a carry and a first step exist)."""
    T, B, H, K = 3, 2, 8, 5
    x, layer, dout = L.make_case(T, B, H, K)
    layer["weight_hh"][:] = 0
    good = L.layer_step(x, layer, dout, rounding=True)
    exact, bound = L.cell_backward_bound(dout, good["act"])
    assert np.all(np.abs(good["dgates"] - exact) <= bound)  # (the restatement's bf16 store: within half a step)
    assert np.all(bound <= 2.0 ** -8 * np.abs(exact) * 1.001 + 1e-5 * np.abs(dout).max())  # the float32 part is small beside the store's
    bad = L.layer_step(x, layer, dout, rounding=True, defect=defect)
    assert np.any(np.abs(bad["dgates"] - exact) > bound)


def test_cell_backward_bound_needs_no_recurrence_for_T1():
    x, layer, dout = L.make_case(1, 3, 8, 5)
    good = L.layer_step(x, layer, dout, rounding=True)
    exact, bound = L.cell_backward_bound(dout, good["act"])
    assert np.all(np.abs(good["dgates"] - exact) <= bound)
    assert not np.any(exact[:, :, :, 8:16])  # df = dc c_{-1} f (1 - f) with c_{-1} = 0


@pytest.mark.parametrize("H", [64, 128])
def test_backward_pack_order_round_trips(H):
    n = 2 * 4 * H * H
    seen = np.zeros((2, 4 * H, H), int)
    for i in range(n // 8):
        d, k, col = L.bwd_fragment(i, H)
        assert 0 <= d < 2 and 0 <= k and k + 8 <= 4 * H and 0 <= col < H
        seen[d, k:k + 8, col] += 1
    assert np.all(seen == 1)  # every weight sits in exactly one fragment
    w = np.arange(n, dtype=np.float64).reshape(2, 4 * H, H)
    packed = L.pack_bwd(w)
    assert np.array_equal(L.unpack_bwd(packed, H), w)
    # a lane's 8 values are 8 consecutive gate rows of one column; the 64 lanes of a k-step cover 16 columns x 32 rows; a slice's k-steps
    # follow each other and cover all 4H rows
    assert np.array_equal(packed[:8], w[0, 0:8, 0]) and np.array_equal(packed[8:16], w[0, 0:8, 1])
    assert np.array_equal(packed[16 * 8:16 * 8 + 8], w[0, 8:16, 0])
    assert np.array_equal(packed[512:520], w[0, 32:40, 0])
    assert np.array_equal(packed[(H // 8) * 512:(H // 8) * 512 + 8], w[0, 0:8, 16])
    assert np.array_equal(packed[n // 2:n // 2 + 8], w[1, 0:8, 0])
