"""GPU: the LSTM layer kernel (csrc/lstm.hip), the DeepSpeech2 front end, model, features and eval script against the float64
restatement of tests/deepspeech2_cases.py.

Bounds.  Saturated routing cases: 1e-6 absolute (the saturation residue 1 - sigmoid(16.7) = 5.6e-8 times a handful of steps).
Random-weight cases: relrms(device, exact) <= 2 S with S = relrms(rounding-only, exact) computed here, per case; each test prints
its ratio relrms / S.  conv1 (a float32 direct kernel with a bf16 store) has an element-wise bound, derived at its test."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import deepspeech2_cases as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 64), (2, 1, 64), (7, 3, 128), (5, 17, 128), (3, 2, 1024)]  # (T, B, H)
# the step kernel's code paths by H / 32: 2 -> one wave per batch tile; 4 -> K split over the waves, blocks of 1 k-step; 8 -> blocks
# of 2 (H = 256, not among the shapes above: added, with a B that fills a second workgroup row); 32 -> blocks of 4
EXTRA_SHAPES = [(4, 70, 256)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    return _lib.load()


def run_layer(lib, x, layer, dir_mask=3, chunk=None, B_alloc=None):
    """x (T, B, K) float, layer: the stacked float32 parameters -> (out_f32, out_bf16 as float32, c_final) NumPy arrays."""
    from mindaudio_amd import _lib

    dev = torch.device("cuda")
    T, B, K = x.shape
    H = layer["weight_hh"].shape[2]
    Kpad = (K + 63) // 64 * 64
    p = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in layer.items()}
    wih = torch.empty((2, 4 * H, Kpad), dtype=torch.bfloat16, device=dev)
    whh = torch.empty((2 * 4 * H * H,), dtype=torch.bfloat16, device=dev)
    bias = torch.empty((2, 4 * H), dtype=torch.float32, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ma_lstm_pack_f32(p["weight_ih"].data_ptr(), p["weight_hh"].data_ptr(), p["bias_ih"].data_ptr(), p["bias_hh"].data_ptr(),
                                    K, Kpad, H, wih.data_ptr(), whh.data_ptr(), bias.data_ptr(), s), "pack")
    xb = torch.zeros((T, B, Kpad), dtype=torch.bfloat16, device=dev)
    xb[:, :, :K] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).to(torch.bfloat16)
    chunk = chunk or T
    nbytes = lib.ma_lstm_workspace_bytes(T, B, H, chunk)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = torch.full((T, B, H), float("nan"), dtype=torch.float32, device=dev)
    out_bf = torch.zeros((T, B, H), dtype=torch.bfloat16, device=dev)
    c = torch.full((2, B, H), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.ma_lstm_bidir_bf16(xb.data_ptr(), T, B, Kpad, H, wih.data_ptr(), whh.data_ptr(), bias.data_ptr(), dir_mask, chunk,
                                      out.data_ptr(), out_bf.data_ptr(), c.data_ptr(), ws.data_ptr(), nbytes, s), "lstm")
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_bf.float().cpu().numpy(), c.cpu().numpy()


# ---- routing, near-exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,H", SHAPES + EXTRA_SHAPES)
def test_lstm_routing_saturated(lib, T, B, H):
    x, layer = C.routing_case(T, B, H)
    want, want_c = C.lstm_bidir(x, layer)
    got, got_bf, got_c = run_layer(lib, x, layer)
    err, err_c = np.abs(got - want).max(), np.abs(got_c - want_c).max()
    print("routing (%d, %d, %d): max |out - ref| = %.3g, max |c - ref| = %.3g" % (T, B, H, err, err_c))
    assert err <= 1e-6 and err_c <= 1e-6
    assert np.array_equal(got_bf, C.bf16_round(got).astype(np.float32))  # the bf16 output is the rounding of the float32 one


# ---- one layer against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 160, 1312])
@pytest.mark.parametrize("T,B,H", SHAPES + [(40, 2, 128)] + EXTRA_SHAPES)
def test_lstm_layer_vs_float64(lib, T, B, H, K):
    """K = 1312 runs padded to 1344 columns."""
    layer = C.lstm_layer_params(100 + K + H, K, H)
    x = C.bf16_round(np.random.RandomState(T * 31 + B).normal(0, 1, (T, B, K)))  # a bf16 activation, as every producer leaves it
    exact, _ = C.lstm_bidir(x, layer)
    S = C.relrms(C.lstm_bidir(x, layer, rounding=True)[0], exact)
    got, _, _ = run_layer(lib, x, layer, chunk=3 if T > 3 else None)  # (several projection chunks, the last one short)
    e = C.relrms(got, exact)
    print("layer (T %d, B %d, H %d, K %d): relrms %.3e, rounding-only %.3e, ratio %.2f" % (T, B, H, K, e, S, e / S))
    assert 0 < S < 3e-2
    assert e <= 2 * S


# ---- cell and layer invariants --------------------------------------------------------------------------------------------------------------
def test_cell_state_is_float32(lib):
    """T = 64, forget and input gates saturated open, g saturated to +1: c grows by exactly 1 per step (up to the residue 64 x 1e-14 of
    tanh(40) and 64 x e^-40 of the sigmoids) and ends at 64."""
    T, B, H, K = 64, 2, 64, 64
    x = np.zeros((T, B, K), np.float32)
    layer = dict(weight_ih=np.zeros((2, 4 * H, K), np.float32), weight_hh=np.zeros((2, 4 * H, H), np.float32),
                 bias_ih=np.full((2, 4 * H), 40.0, np.float32), bias_hh=np.zeros((2, 4 * H), np.float32))
    want, want_c = C.lstm_bidir(x, layer)
    assert np.abs(want_c - 64.0).max() <= 1e-9
    got, _, got_c = run_layer(lib, x, layer, chunk=7)
    assert np.abs(got_c - want_c).max() <= 1e-5
    assert np.abs(got - want).max() <= 1e-5


def test_layer_is_sum_of_directions_and_repeats_bit_for_bit(lib):
    for T in (6, 7):  # even, and odd: the middle frame is served by both directions in one launch
        layer = C.lstm_layer_params(7, 64, 128)
        x = np.random.RandomState(T).normal(0, 1, (T, 3, 64))
        both, both_bf, c = run_layer(lib, x, layer)
        again, again_bf, c2 = run_layer(lib, x, layer)
        assert np.array_equal(both, again) and np.array_equal(both_bf, again_bf) and np.array_equal(c, c2)
        fwd, _, cf = run_layer(lib, x, layer, dir_mask=1)
        bwd, _, cb = run_layer(lib, x, layer, dir_mask=2)
        assert np.array_equal(both, fwd + bwd)
        assert np.array_equal(c[0], cf[0]) and np.array_equal(c[1], cb[1])
        assert not np.array_equal(fwd, bwd)


def test_batch_rows_are_independent(lib):
    layer = C.lstm_layer_params(8, 160, 128)
    x = np.random.RandomState(9).normal(0, 1, (5, 3, 160))
    three, _, _ = run_layer(lib, x, layer)
    alone, _, _ = run_layer(lib, x[:, :1], layer)
    assert np.array_equal(three[:, :1], alone)


def test_abi_refusals(lib):
    from mindaudio_amd import _lib

    assert lib.ma_lstm_workspace_bytes(4, 2, 96, 4) == _lib.MA_ERR_UNSUPPORTED
    dev = torch.device("cuda")
    buf = torch.zeros((1 << 20,), dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    args = lambda H, Kpad, ws: (p, 4, 2, Kpad, H, p, p, p, 3, 4, p, p, None, p, ws, None)  # noqa: E731
    assert lib.ma_lstm_bidir_bf16(*args(96, 64, 1 << 20)) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_lstm_bidir_bf16(*args(64, 96, 1 << 20)) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_lstm_bidir_bf16(*args(64, 64, 16)) == _lib.MA_ERR_WORKSPACE
    assert lib.ma_lstm_pack_f32(p, p, p, p, 64, 64, 96, p, p, p, None) == _lib.MA_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---- front end ----------------------------------------------------------------------------------------------------------------------------
def _model(cfg, state):
    from mindaudio_amd.models import DeepSpeechModel

    m = DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                        audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))
    m.load_weights(state)
    return m.cuda().eval()


_FRONT = {}


def _front_model(F):
    if F not in _FRONT:
        cfg = dict(sample_rate=1600 if F == 17 else 16000, window_size=0.02, H=64, layers=1, B=3, T=22)
        state = C.make_state(cfg, 20 + F)
        _FRONT[F] = (cfg, state, _model(cfg, state))
    return _FRONT[F]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [21, 22])
@pytest.mark.parametrize("F", [17, 161])
def test_front_end_stages(lib, F, T, B):
    cfg, state, model = _front_model(F)
    x = C.make_input(cfg, 5 * T + B, B=B, T=T, pad_frames=4)
    xin = model.frontend(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    F1, T1 = (F - 1) // 2 + 1, (T - 1) // 2 + 1
    F2 = (F1 - 1) // 2 + 1
    ws = [w for w in model._ws.values() if w["xin"] is xin][0]
    act1 = ws["act1"].float().cpu().numpy().reshape(T1 + 10, B, ws["Fpad"], 32)

    # stage 1: conv1 + BN + tanh.  Pre-activation z = scale * acc + shift with acc a float32 fmaf chain over 451 taps:
    # |acc - exact| <= 451 * 2^-24 * sum |w x| (each of the 451 roundings is at most half an ulp of a partial sum <= sum |terms|),
    # |z error| <= |scale| * that + 2 * 2^-24 |z| (the fold's two float32 constants and the final fmaf); tanh is 1-Lipschitz and
    # tanhf is good to a few ulp (4 * 2^-24 taken); the bf16 store (8 significant bits) adds half an ulp, at most 2^-8 relative.
    exact1 = C.mask_conv(state, x, stage1_only=True)                                 # (B, 32, F1, T1)
    scale = np.asarray(state["conv.bn1.gamma"], np.float64) / np.sqrt(np.asarray(state["conv.bn1.moving_variance"], np.float64) + 1e-5)
    terms = C.conv1_abs_terms(state, x)
    bound = (451 * 2.0 ** -24 * terms * np.abs(scale)[None, :, None, None] + 6 * 2.0 ** -24 * (1 + np.abs(np.arctanh(np.clip(exact1, -0.999999, 0.999999))))
             + 2.0 ** -8 * np.abs(exact1))
    got1 = act1[5:5 + T1, :, 10:10 + F1, :].transpose(1, 3, 2, 0)                   # -> (B, 32, F1, T1)
    excess = (np.abs(got1 - exact1) - bound).max()
    print("conv1 F %d T %d B %d: max |err| %.3e, max (|err| - bound) %.3e" % (F, T, B, np.abs(got1 - exact1).max(), excess))
    assert excess <= 0
    mask = np.ones_like(act1, dtype=bool)
    mask[5:5 + T1, :, 10:10 + F1, :] = False
    assert np.all(act1[mask] == 0)  # halo frames and padding rows stay zero

    # stage 2 (the whole MaskConv): 2 x rounding-only
    exact = C.rnn_input(C.mask_conv(state, x))                                        # (T1, B, 32 F2), feature c * F2 + f
    S = C.relrms(C.rnn_input(C.mask_conv(state, x, rounding=True)), exact)
    got = xin.float().cpu().numpy()
    assert got.shape == (T1, B, (32 * F2 + 63) // 64 * 64) and np.all(got[:, :, 32 * F2:] == 0)
    got = got[:, :, :32 * F2].reshape(T1, B, F2, 32).transpose(0, 1, 3, 2).reshape(T1, B, 32 * F2)  # f * 32 + c -> c * F2 + f
    e = C.relrms(got, exact)
    print("MaskConv F %d T %d B %d: relrms %.3e, rounding-only %.3e, ratio %.2f" % (F, T, B, e, S, e / S))
    assert 0 < S < 3e-2 and e <= 2 * S
    # nothing is masked: the frames that lie wholly inside the zero padding come out non-zero, as the reference's would
    assert np.abs(got[T1 - 1]).max() > 1e-3 and np.abs(exact[T1 - 1]).max() > 1e-3


# ---- model --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "yaml-geometry"])
def test_model_vs_float64(lib, name):
    cfg, state, x, exact, rounded = C.model_case(name)
    S = C.relrms(rounded, exact)
    model = _model(cfg, state)
    lengths = np.array([cfg["T"], cfg["T"] - 6, 1][:cfg["B"]], np.int32)
    logits, out_len = model(x, lengths)  # NumPy in
    assert tuple(logits.shape) == exact.shape and logits.dtype == torch.float32
    assert np.array_equal(np.asarray(out_len), C.get_seq_lens(lengths))
    e = C.relrms(logits.cpu().numpy(), exact)
    print("model %s: relrms %.3e, rounding-only %.3e, ratio %.2f" % (name, e, S, e / S))
    assert 0 < S < 3e-2 and e <= 2 * S
    probs, out_len2 = model.predict(torch.from_numpy(x).cuda(), lengths)
    assert tuple(probs.shape) == (cfg["B"], exact.shape[0], len(C.LABELS)) and np.array_equal(out_len2, out_len)
    p = probs.cpu().numpy().astype(np.float64)
    assert np.abs(p.sum(-1) - 1).max() <= 1e-5  # 29 float32 terms: 29 * 2^-24 = 1.7e-6, and the division
    assert np.abs(p - C.softmax_btc(logits.cpu().numpy().astype(np.float64))).max() <= 1e-6
    if name == "small":
        # the stale-weights trap: weights loaded after a forward must be used
        state2 = C.make_state(cfg, 99)
        model.load_weights(state2)
        logits2, _ = model(x, lengths)
        exact2 = C.forward(state2, cfg, x)[0]
        assert C.relrms(logits2.cpu().numpy(), exact2) <= 2 * C.relrms(C.forward(state2, cfg, x, rounding=True)[0], exact2)
        assert C.relrms(logits2.cpu().numpy(), exact) > 0.5


# ---- features -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_parse_audio_vs_numpy(lib, normalize):
    """Bound: the magnitude is within 2e-5 of its maximum (test_feature_post.py's bound for magphase of an stft); log1p is
    1-Lipschitz, and the normalisation divides the error by the standard deviation."""
    from mindaudio_amd.deepspeech2.dataset import LoadAudioAndTranscript

    loader = LoadAudioAndTranscript(dict(sample_rate=16000, window_size=0.02, window_stride=0.01), normalize=normalize)
    got = loader.parse_audio(C.WAV)
    from oracle.speech_features import read_wav

    wave, _ = read_wav(C.WAV)
    want, mag = C.parse_audio(wave, 16000, 0.02, 0.01, normalize)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape == (161, 1 + len(wave) // 160)
    bound = 2e-5 * mag.max() / (np.log1p(mag).std() if normalize else 1.0)
    err = np.abs(got.cpu().numpy() - want).max()
    print("parse_audio normalize=%s: max |err| %.3e, bound %.3e" % (normalize, err, bound))
    assert err <= bound + 2.0 ** -23 * np.abs(want).max()  # (and the float32 store of the result)


# ---- eval end to end ------------------------------------------------------------------------------------------------------------------------
def _write_manifest(tmp_path, waves, texts, name):
    from scipy.io import wavfile

    samples = []
    for i, (w, text) in enumerate(zip(waves, texts)):
        if isinstance(w, str):
            wav_path = w
        else:
            wav_path = str(tmp_path / ("%s%d.wav" % (name, i)))
            wavfile.write(wav_path, 16000, (w * 32767).astype(np.int16))
        with open(tmp_path / ("%s%d.txt" % (name, i)), "w") as fh:
            fh.write(text + "\n")
        samples.append({"wav_path": wav_path, "transcript_path": "%s%d.txt" % (name, i)})
    path = tmp_path / (name + ".json")
    path.write_text(json.dumps({"root_path": str(tmp_path), "samples": samples}))
    return str(path)


def _config(manifest, sample_rate, H, layers, batch):
    return {"SpectConfig": dict(sample_rate=sample_rate, window_size=0.02, window_stride=0.01, window="hamming"),
            "ModelConfig": dict(rnn_type="LSTM", hidden_size=H, hidden_layers=layers),
            "EvalConfig": dict(batch_size=batch, test_manifest=manifest), "Pretrained_model": "", "labels": C.LABELS}


def test_eval_prescribed_probabilities(lib, tmp_path):
    from mindaudio_amd.deepspeech2.eval import evaluate

    g = np.random.RandomState(0)
    waves = [C.WAV, 0.1 * g.normal(0, 1, 8000), 0.1 * g.normal(0, 1, 12000)]
    refs = ["THE CAT SAT", "HI YOU", "A B"]
    frames = ["TTHHE_E  CA_T _SAAT", "HI_ _YO", "A__ BB_C"]  # -> "THEE CAT SAT" (CER 1/9), "HI YO" (1 word, 1 char), "A BC"
    manifest = _write_manifest(tmp_path, waves, refs, "p")
    calls = []

    def model(inputs, input_length):
        assert tuple(inputs.shape) == (3, 1, 161, 3500) and inputs.is_cuda
        assert input_length.tolist() == [600.0, 51.0, 76.0]
        calls.append(1)
        probs = torch.full((3, 1750, len(C.LABELS)), 0.001)
        for b, fr in enumerate(frames):
            ids = [C.LABELS.index(ch) for ch in fr] + [C.LABELS.index("Q")] * (1750 - len(fr))  # past `size`: never decoded
            probs[b, torch.arange(1750), torch.tensor(ids)] = 0.9
        return probs.cuda(), np.array([len(fr) for fr in frames], np.int32)

    lines = []
    wer, cer = evaluate(_config(manifest, 16000, 64, 1, 3), model=model, log=lambda *a: lines.append(" ".join(str(v) for v in a)))
    assert calls == [1]
    assert lines[0:3] == ["Ref: the cat sat", "Hyp: thee cat sat", "WER: %s CER: %s \n" % (1 / 3, 1 / 9)]
    assert lines[3:6] == ["Ref: hi you", "Hyp: hi yo", "WER: 0.5 CER: 0.2 \n"]
    assert lines[6:9] == ["Ref: a b", "Hyp: a bc", "WER: 0.5 CER: 0.5 \n"]
    assert (wer, cer) == (3 / 7, 3 / 16)
    assert lines[9] == "Test Summary \tAverage WER 42.857\tAverage CER 18.750\t" and len(lines) == 10


def test_eval_real_small_model(lib, tmp_path):
    from mindaudio_amd.deepspeech2 import eval as ds2_eval
    from mindaudio_amd.utils import ckpt

    g = np.random.RandomState(1)
    waves = [0.1 * g.normal(0, 1, n) for n in (4000, 6000, 3000)]
    manifest = _write_manifest(tmp_path, waves, ["AB C", "HELLO", "Q"], "r")
    cfg = dict(sample_rate=1600, window_size=0.02, H=64, layers=2, B=2, T=45)
    config = _config(manifest, 1600, 64, 2, 2)
    path = str(tmp_path / "small.ckpt")
    ckpt.write_mindspore_ckpt(path, C.make_state(cfg, 3))
    config["Pretrained_model"] = path
    lines = []
    wer, cer = ds2_eval.evaluate(config, log=lambda *a: lines.append(" ".join(str(v) for v in a)))
    assert lines[0] == "Successfully loading the pre-trained model"
    assert sum(l.startswith("Ref:") for l in lines) == 4  # two bins of two: the last one refilled from the tail
    import re

    m = re.fullmatch(r"Test Summary \tAverage WER (\d+\.\d{3})\tAverage CER (\d+\.\d{3})\t", lines[-1])
    assert m and abs(float(m.group(1)) - wer * 100) <= 5e-4 and abs(float(m.group(2)) - cer * 100) <= 5e-4
