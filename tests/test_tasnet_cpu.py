"""CPU: the float64 restatement of tests/tasnet_cases.py against independent statements of the same arithmetic (torch.nn.LSTM, a
literal transcription of the reference's loss), the checkpoint names, the data pipeline, and the conditions under which the GPU
tests' yardsticks mean something."""
import json
import os

import numpy as np
import pytest
import torch

import tasnet_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the restated stack against torch.nn.LSTM ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,H,K", [(5, 3, 16, 24), (1, 1, 8, 8)])
def test_stack_restatement_equals_torch_lstm(T, B, H, K):
    layers = C.stack_params(5, K, H, 4)
    x = np.random.RandomState(6).normal(0, 1, (T, B, K))
    ref = torch.nn.LSTM(K, H, num_layers=4).double()
    with torch.no_grad():
        for l, p in enumerate(layers):
            for n, v in p.items():
                getattr(ref, "%s_l%d" % (n, l)).copy_(torch.from_numpy(v.astype(np.float64)))
        want, (hn, cn) = ref(torch.from_numpy(x))
    got, h_final, c_final = C.lstm_stack(x, layers)
    assert np.abs(got - want.numpy()).max() <= 1e-12
    assert np.abs(h_final - hn.numpy()).max() <= 1e-12 and np.abs(c_final - cn.numpy()).max() <= 1e-12


# ---- Separation_Loss ------------------------------------------------------------------------------------------------------------------------
def _reference_loss(source, estimate_source, source_lengths):
    """mindaudio/loss/separation_loss.py:56-130 line by line with NumPy in place of the MindSpore ops (float64)."""
    EPS = 1e-8
    B, Cn, _, L = source.shape
    num_samples = (L * source_lengths).reshape(-1, 1, 1, 1).astype(np.float64)
    mean_target = source.sum((2, 3), keepdims=True) / num_samples
    mean_estimate = estimate_source.sum((2, 3), keepdims=True) / num_samples
    zero_mean_target = source - mean_target
    zero_mean_estimate = estimate_source - mean_estimate
    flat_target = zero_mean_target.reshape(B, Cn, -1)
    flat_estimate = zero_mean_estimate.reshape(B, Cn, -1)
    s_target = flat_target[:, None]       # [B, 1, C, T]
    s_estimate = flat_estimate[:, :, None]  # [B, C, 1, T]
    pair_wise_dot = (s_estimate * s_target).sum(3, keepdims=True)
    s_target_energy = (s_target ** 2).sum(3, keepdims=True) + EPS
    pair_wise_proj = pair_wise_dot * s_target / s_target_energy
    e_noise = s_estimate - pair_wise_proj
    pair_wise_si_snr = (pair_wise_proj ** 2).sum(3) / ((e_noise ** 2).sum(3) + EPS)
    pair_wise_si_snr = 10 * np.log(pair_wise_si_snr + EPS) / np.log(10.0)
    perms = np.array([[0, 1], [1, 0]])
    perms_one_hot = np.array([[1, 0], [0, 1], [0, 1], [1, 0]], np.float64)
    snr_set = pair_wise_si_snr.reshape(B, -1) @ perms_one_hot
    max_snr_idx = snr_set.argmax(1)
    max_snr = snr_set.max(1, keepdims=True) / Cn
    max_snr_perm = perms[max_snr_idx, :]
    reorder_source = np.zeros_like(estimate_source)
    for b in range(B):
        for c in range(Cn):
            reorder_source[b, c] = estimate_source[b, 1] if max_snr_perm[b][c] == 1 else estimate_source[b, 0]
    return 0 - max_snr.mean(), max_snr, max_snr_perm, reorder_source


def test_separation_loss_restatement_equals_the_reference_formulae():
    g = np.random.RandomState(3)
    B, K, L = 3, 7, 8
    source = g.normal(0, 1, (B, 2, K, L)) + 0.3  # (a mean, so that the division by the length matters)
    estimate = source + 0.3 * g.normal(0, 1, source.shape)
    estimate[1] = estimate[1, ::-1]  # utterance 1: the swapped permutation wins
    for lengths in (np.array([K, K, K]), np.array([K, 4, 5])):  # the example's only value, and source_lengths < K
        want = _reference_loss(source, estimate, lengths)
        got = C.separation_loss(source, estimate, lengths)
        assert abs(got[0] - want[0]) <= 1e-9 and np.abs(got[1] - want[1]).max() <= 1e-9
        assert np.array_equal(got[2], want[2]) and got[2].tolist() == [[0, 1], [1, 0], [0, 1]]
        assert np.array_equal(got[3], want[3])
    # the short length changes the means and with them the value: the case is not vacuous
    assert abs(C.separation_loss(source, estimate, [K, 4, 5])[0] - C.separation_loss(source, estimate, [K, K, K])[0]) > 1e-3


# ---- checkpoint names -------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_names_round_trip(tmp_path):
    from mindaudio_amd.models import TasNet
    from mindaudio_amd.utils import ckpt

    cfg = dict(L=8, N=24, H=64, layers=2, nspk=2)
    state = C.make_state(cfg, 4)
    model = TasNet(cfg["L"], cfg["N"], cfg["H"], cfg["layers"])
    assert sorted(model.state_dict()) == sorted(C.param_shapes(**cfg))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == C.param_shapes(**cfg)
    model.load_weights(state)
    g = np.random.RandomState(0)
    new_lstm = (g.normal(0, 1, (512, 500)).astype(np.float32), g.normal(0, 1, (512,)).astype(np.float32))
    ref = ckpt.tasnet_to_reference_names(model.state_dict(), new_lstm=new_lstm)
    assert ref["encoder.conv1d_U.weight"].shape == (24, 8, 1, 1)  # MindSpore's Conv1d keeps a unit axis
    assert np.array_equal(ref["separator.new_lstm.weight"], new_lstm[0]) and ref["separator.new_lstm.bias"].shape == (512,)
    assert ckpt.tasnet_to_reference_names(model.state_dict())["separator.new_lstm.weight"].shape == (512, 500)
    path = str(tmp_path / "tasnet.ckpt")
    ckpt.write_mindspore_ckpt(path, dict(ref, **{"moments.separator.fc.weight": np.zeros((48, 64), np.float32), "global_step": np.array(3)}))
    back = ckpt.convert_tasnet_names(ckpt.read_mindspore_ckpt(path))
    assert sorted(back) == sorted(state)  # new_lstm and the optimizer state are gone
    for k, v in state.items():
        assert np.array_equal(back[k], v), k
    fresh = TasNet(cfg["L"], cfg["N"], cfg["H"], cfg["layers"])
    missing, unexpected = ckpt.load_mindspore_checkpoint(fresh, path)
    assert missing == [] and unexpected == []
    for k, v in fresh.state_dict().items():
        assert np.array_equal(v.numpy(), state[k]), k
    with pytest.raises(NotImplementedError, match="reference cannot run it either"):
        TasNet(8, 24, 64, 2, bidirectional=True)
    with pytest.raises(ValueError):
        TasNet(8, 24, 64, 2, schedule="eager")


# ---- data -------------------------------------------------------------------------------------------------------------------------------------
def test_dataset_generator_order_padding_shapes(tmp_path):
    from mindaudio_amd.tasnet import DatasetGenerator

    waves = C.write_dataset(str(tmp_path), [900, 1300, 900], ["b", "a", "c"])
    ds = DatasetGenerator(str(tmp_path), 2, sample_rate=8000, L=40)
    assert len(ds) == 3
    # (#samples, path) descending: the longest first, then the two of 900 samples in REVERSE path order
    for i, name in enumerate(["a", "c", "b"]):
        mixture, n, sources = ds[i]
        assert mixture.shape == (3320, 40) and mixture.dtype == np.float32 and sources.shape == (2, 3320, 40) and n == 3320
        mix, s1, s2 = waves[name]
        assert np.array_equal(mixture.reshape(-1)[:len(mix)], mix) and not mixture.reshape(-1)[len(mix):].any()
        assert np.array_equal(sources[0].reshape(-1)[:len(s1)], s1) and np.array_equal(sources[1].reshape(-1)[:len(s2)], s2)
        assert not sources.reshape(2, -1)[:, len(s1):].any()
    small = DatasetGenerator(str(tmp_path), 1, L=8, segments=200)
    assert small[0][0].shape == (200, 8) and small[0][1] == 200
    with pytest.raises(ValueError):
        DatasetGenerator(str(tmp_path), 1, L=8, segments=100)  # 800 samples: shorter than every utterance


def test_yaml_settings_fixture_matches_the_documented_geometry():
    with open(os.path.join(HERE, "golden", "tasnet_yaml_settings.json")) as fh:
        y = json.load(fh)
    assert (y["batch_size"], y["bidirectional"], y["hidden_size"], y["num_layers"], y["N"], y["L"], y["nspk"]) == (1, 0, 512, 4, 500, 40, 2)
    g = C.YAML_GEOMETRY
    assert (g["L"], g["N"], g["H"], g["layers"], g["nspk"]) == (y["L"], y["N"], y["hidden_size"], y["num_layers"], y["nspk"])


# ---- the yardsticks' conditions -------------------------------------------------------------------------------------------------------------------
STACK_TABLE = [(1, 1, 64, 64, 4), (2, 2, 64, 40, 4), (3, 1, 128, 64, 1), (19, 3, 64, 40, 4), (7, 17, 128, 160, 3), (5, 70, 256, 64, 2),
               (12, 1, 512, 500, 4)]  # (T, B, H, K, layers) of test_tasnet_gpu.py


@pytest.mark.parametrize("T,B,H,K,layers", STACK_TABLE)
def test_stack_yardsticks_are_inside_their_condition(T, B, H, K, layers):
    _, _, exact, rounded = C.stack_case(T, B, H, K, layers)
    S = C.relrms(rounded[0], exact[0])
    print("stack (T %d, B %d, H %d, K %d, %d layers): S = %.2e" % (T, B, H, K, layers, S))
    assert 1e-4 < S < 3e-2


@pytest.mark.parametrize("name", ["small", "tiny", "yaml-geometry"])
def test_model_yardsticks_are_inside_their_condition(name):
    cfg, state, x, exact, rounded, h, hr = C.model_case(name)
    S, S_h = C.relrms(rounded, exact), C.relrms(hr, h)
    print("model %s: S(est_source) = %.2e, S(stack output) = %.2e" % (name, S, S_h))
    assert 1e-4 < S < 3e-2 and 1e-4 < S_h < 3e-2
    assert exact.shape == (cfg["B"], cfg["nspk"], cfg["K"], cfg["L"])
    assert not exact[-1, :, -1].any()  # the all-zero segment comes out as zeros (norm_coef = 0 multiplies the bias too)
    if name == "small":  # why the model cases draw the fc weight at 32 x Xavier gain
        plain = C.make_state(cfg, 21, fc_gain=1.0)
        S1 = C.relrms(C.forward(plain, cfg, x, rounding=True)[0], C.forward(plain, cfg, x)[0])
        print("model small at plain Xavier gain: S = %.2e" % S1)
        assert S1 < 1e-4


@pytest.mark.parametrize("T,layers", [(1, 4), (4, 4), (7, 3)])
@pytest.mark.parametrize("H", [64, 128])
def test_saturated_stack_case_is_saturated_in_every_layer(T, layers, H):
    x, p = C.stack_routing_case(T, 3, H, layers)
    for rounding in (False, True):
        stats = []
        out, _, c = C.lstm_stack(x, p, rounding=rounding, stats=stats)
        assert len(stats) == layers and all(len(s) == T for s in stats)
        assert min(min(s) for s in stats) >= (16.7 if not rounding else 16.2)
    assert np.abs(out).max() > 0.7 and np.abs(np.round(c) - c).max() < 1e-5  # c moves in whole steps
    # the layers do not repeat each other: a wrong layer's weights would show
    assert not np.array_equal(p[0]["weight_hh"], p[-1]["weight_hh"]) or layers == 1
