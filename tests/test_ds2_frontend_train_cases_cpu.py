"""CPU: the float64 restatement of train-mode MaskConv (ds2_frontend_train_cases) against torch.autograd, the planted defects against
the comparators that the GPU tests use, and what of models.DeepSpeech2Trainer(frontend="trained") exists without a device."""
import numpy as np
import pytest
import torch

import deepspeech2_cases as C
import ds2_frontend_train_cases as FE


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_restatement_equals_float64_autograd():
    cfg, state, x, dout, exact, _, _, fwd, _ = FE.case("small")
    out, grads, moving = FE.autograd(state, x, dout)
    assert _rel(fwd["out"], out) < 1e-10
    for name in FE.PARAMS:
        assert exact[name].shape == grads[name].shape and _rel(exact[name], grads[name]) < 1e-10, name
    for name, want in moving.items():  # (torch's batch_norm: the unbiased variance into the running one, as restated)
        assert _rel(fwd["moving"][name], want) < 1e-10, name


def test_row_forms_of_the_conv2_gradients_equal_the_closed_forms():
    """The device's formulation - parity images, 12-row runs, reversed taps, the dropped 22nd row - is the same sum."""
    cfg, state, x, dout, exact, _, _, fwd, _ = FE.case("small")
    w2 = np.asarray(state["conv.conv2.weight"], np.float64)
    assert _rel(FE.conv2_dx_by_rows(exact["dz2"], w2, fwd["act1"].shape[2]), exact["dact1"]) < 1e-12
    assert _rel(FE.conv2_dw_by_rows(exact["dz2"], fwd["act1"]), exact["conv.conv2.weight"]) < 1e-12


@pytest.mark.parametrize("name", ["small", "yaml-geometry"])
def test_yardstick_conditions_hold_for_the_restatement_alone(name):
    """0 < S < 5e-2 and cosine >= 0.99 for every parameter: conditions of the GPU tests that do not depend on the device."""
    cfg, state, x, dout, exact, rounded, S, fe, fr = FE.case(name)
    for n in FE.PARAMS:
        cos = FE.cosine(rounded[n], exact[n])
        print("%-14s %-20s S %.3e cosine %.6f" % (name, n, S[n], cos))
        assert 0 < S[n] < 5e-2 and cos >= 0.99, n
    s_out = C.relrms(fr["out"], fe["out"])
    print("%-14s xin S %.3e" % (name, s_out))
    assert 0 < s_out < 5e-2


TOUCHES = {"stats_constant": ("conv.conv1.weight", "conv.conv2.weight", "conv.bn1.gamma"),
           "xhat_term_dropped": ("conv.conv1.weight", "conv.conv2.weight"),
           "taps_not_reversed": ("conv.conv1.weight", "conv.bn1.gamma", "conv.bn1.beta"),
           "parity_swapped": ("conv.conv1.weight", "conv.bn1.gamma", "conv.bn1.beta"),
           "row22_kept": ("conv.conv2.weight",)}


@pytest.mark.parametrize("defect", sorted(TOUCHES))
def test_planted_defects_land_above_the_bound(defect):
    """The GPU comparator is relrms(device, exact) <= 2 S per parameter: a restatement with the defect planted, in the rounding-only
    form, must fail it for every parameter the defect touches."""
    cfg, state, x, dout, exact, _, S, _, fr = FE.case("small")
    bad = FE.backward(state, fr, dout, defect=defect)
    for n in TOUCHES[defect]:
        e = C.relrms(bad[n], exact[n])
        print("%-18s %-20s relrms %.3e, 2 S %.3e" % (defect, n, e, 2 * S[n]))
        assert e > 2 * S[n], (defect, n)


def test_unbiased_variance_for_normalising_is_rejected_by_the_statistics_comparator():
    """count / (count - 1) - 1 is 1.6e-3 here and smaller on larger shapes: below bf16's step, so the 2 S bounds cannot see it.  The
    statistics comparator (12 u E[y^2]) does, and it is the check that the GPU test makes of the variance."""
    cfg, state, x, dout, _, _, _, fe, _ = FE.case("small")
    for y, bn in ((fe["y1"], fe["bn1"]), (fe["y2"], fe["bn2"])):
        assert FE.stats_failures(bn["mean"], bn["var"], y, 1) == []
        assert FE.stats_failures(bn["mean"], bn["unbiased"], y, 1) != []
    bad = FE.forward(state, x, defect="unbiased_normalise")
    assert C.relrms(bad["out"], fe["out"]) > 0


def test_conv1_dw_abs_terms_bounds_the_gradient():
    cfg, state, x, dout, exact, _, _, _, _ = FE.case("small")
    terms = FE.conv1_dw_abs_terms(x, exact["dz1"])
    assert terms.shape == (32, 1, 41, 11) and np.all(np.abs(exact["conv.conv1.weight"]) <= terms * (1 + 1e-12))


def test_device_layout_helpers_round_trip():
    a = np.random.RandomState(0).normal(size=(3, 32, 5, 23))
    assert np.array_equal(FE.from_device_xin(FE.to_device_xin(a, 192), 5), a)
    assert not np.any(FE.to_device_xin(a, 192)[:, :, 160:])
    assert np.array_equal(FE.from_channel_last(FE.to_channel_last(a)), a)


# ---- construction and binding: these fail on a tree without the trained front end ----------------------------------------------------------
def _model():
    from mindaudio_amd.models import DeepSpeechModel

    cfg = C.SMALL
    return DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                           audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))


def test_trainer_constructs_with_a_trained_front_end():
    from mindaudio_amd.models import DeepSpeech2Trainer

    tr = DeepSpeech2Trainer(_model(), 3e-4, 1e-5, frontend="trained")
    assert tr.frontend == "trained" and tr._names()[-6:] == list(FE.PARAMS)
    frozen = DeepSpeech2Trainer(_model(), 3e-4, 1e-5)
    assert frozen.frontend == "frozen" and not any(n.startswith("conv.") for n in frozen._names())
    with pytest.raises(ValueError):
        DeepSpeech2Trainer(_model(), 3e-4, 1e-5, frontend="other")
    with pytest.raises(NotImplementedError, match="frontend"):
        DeepSpeech2Trainer(_model(), 3e-4, 1e-5, train_conv=True)


def test_new_symbols_are_bound():
    from mindaudio_amd import _lib, ops

    lib = _lib.load()
    for name in ("ma_ds2_conv1_raw_f32", "ma_ds2_conv1_raw_parts", "ma_ds2_bn_stats_f32", "ma_ds2_stats_parts", "ma_ds2_bn_finalize_f32",
                 "ma_ds2_bn_tanh_fwd_bf16", "ma_ds2_bn_tanh_bwd_f32", "ma_ds2_bn_tanh_bwd_workspace_bytes", "ma_ds2_conv1_dw_f32",
                 "ma_ds2_conv1_dw_parts", "ma_ds2_commit_f32"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 4
    assert callable(ops.ds2_frontend_train) and callable(ops.ds2_frontend_backward)
    # the host-side plans: partial counts and refusals, no device needed
    assert lib.ma_ds2_conv1_raw_parts(3, 45) == 9 and lib.ma_ds2_conv1_dw_parts(3, 45, 0) == 69 and lib.ma_ds2_conv1_dw_parts(3, 45, 2) == 35
    assert lib.ma_ds2_conv1_dw_parts(64, 1250, 0) == 1000  # 40 frames per workgroup: the chain of 40 * 81 in the kernel's header
    assert lib.ma_ds2_stats_parts(33) < 0 and lib.ma_ds2_bn_tanh_bwd_workspace_bytes(4, 33) < 0


def test_transposed_conv2_weight_images():
    """ops.ds2_frontend_operands on the CPU: W_p[ci, j', k * 32 + co] = w2[co, ci, p + 2 (10 - k), 10 - j'], zero where no such tap."""
    from mindaudio_amd import ops

    m = _model()
    P = ops.ds2_frontend_operands(m)
    w2 = m.conv.conv2.weight.detach()
    want = torch.zeros((2, 32, 11, 12, 32))
    for p in (0, 1):
        for k in range(11):
            if p + 2 * (10 - k) <= 20:
                want[p, :, :, k, :] = w2[:, :, p + 2 * (10 - k), :].flip(2).permute(1, 2, 0)
    assert torch.equal(P["w2t"].view(2, 32, 11, 12, 32), want.to(torch.bfloat16))
    assert P["w1t"].shape == (451, 32) and torch.equal(P["w1t"].t().reshape(32, 1, 41, 11), m.conv.conv1.weight.detach())
