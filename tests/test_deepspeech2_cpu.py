"""CPU: the float64 restatement of DeepSpeech2 (tests/deepspeech2_cases.py) against independent statements of the same arithmetic
(torch.nn.LSTM, torch.nn.functional.conv2d, hand-worked decoder and error-rate cases), and the host-side parts of the product:
BatchNorm fold, W_ih column permutation, lengths, checkpoint names, decoder, dataset batching.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import deepspeech2_cases as C


# ---- restatement vs torch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,K,H", [(1, 1, 64, 64), (7, 3, 160, 64), (5, 2, 1312, 128)])
def test_lstm_loop_equals_torch_lstm(T, B, K, H):
    layer = C.lstm_layer_params(3, K, H)
    x = np.random.RandomState(4).normal(0, 1, (T, B, K))
    ref = torch.nn.LSTM(K, H, bidirectional=True).double()
    with torch.no_grad():
        for d, suffix in enumerate(("", "_reverse")):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(ref, n + "_l0" + suffix).copy_(torch.from_numpy(layer[n][d].astype(np.float64)))
        y, (_, cn) = ref(torch.from_numpy(x))
    want = y.reshape(T, B, 2, H).sum(2).numpy()  # deepspeech2.py:183-186
    got, c = C.lstm_bidir(x, layer)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(c - cn.numpy()).max() <= 1e-12
    fwd, _ = C.lstm_bidir(x, layer, dirs=(0,))
    assert np.abs(fwd - y[:, :, :H].numpy()).max() <= 1e-12


@pytest.mark.parametrize("F", [17, 161])
@pytest.mark.parametrize("T", [21, 22])
def test_conv_restatement_equals_torch_conv2d(F, T):
    g = np.random.RandomState(F + T)
    x = g.normal(0, 1, (2, 1, F, T))
    w1, w2 = g.normal(0, 0.1, (32, 1, 41, 11)), g.normal(0, 0.1, (32, 32, 21, 11))
    y1 = C.conv2d(x, w1, (2, 2), (20, 5))
    want1 = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w1), stride=(2, 2), padding=(20, 5))
    assert y1.shape == tuple(want1.shape) == (2, 32, (F - 1) // 2 + 1, (T - 1) // 2 + 1)
    assert np.abs(y1 - want1.numpy()).max() <= 1e-12 * 451
    y2 = C.conv2d(y1, w2, (2, 1), (10, 5))
    want2 = torch.nn.functional.conv2d(want1, torch.from_numpy(w2), stride=(2, 1), padding=(10, 5))
    assert y2.shape == tuple(want2.shape)
    assert np.abs(y2 - want2.numpy()).max() <= 1e-12 * np.abs(want2.numpy()).max() * 100


def test_routing_cases_are_saturated():
    for T, B, H in [(1, 1, 64), (2, 1, 64), (7, 3, 128), (5, 17, 128), (3, 2, 1024), (4, 70, 256)]:
        x, layer = C.routing_case(T, B, H)
        stats = []
        out, _ = C.lstm_bidir(x, layer, stats=stats)
        assert min(stats) >= 16.7, (T, B, H, min(stats))
        assert np.abs(out).max() > 0.7  # (not all zero: the pattern moves)
        for a in (x, layer["weight_ih"], layer["weight_hh"], layer["bias_ih"]):
            assert np.array_equal(C.bf16_round(a), a.astype(np.float64))  # exact in bf16


# ---- host-side helpers of the product ---------------------------------------------------------------------------------------------------------
def _model(cfg):
    from mindaudio_amd.models import DeepSpeechModel

    return DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                           audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))


def test_get_seq_lens_and_geometry():
    m = _model(C.SMALL)
    assert (m.pre, m.stride) == ([-1, -1], [2, 1])
    lens = np.array([1, 2, 21, 22, 3500], np.int32)
    want = np.array([1, 1, 11, 11, 1750], np.int32)  # ((len - 1) / 2 + 1 - 1) / 1 + 1, by hand
    assert np.array_equal(m.get_seq_lens(lens), want) and np.array_equal(C.get_seq_lens(lens), want)
    assert m.get_seq_lens(lens).dtype == np.int32
    assert (m.n_freq, m.rnn_input_size) == (17, 160)
    y = _model(C.YAML_GEOMETRY)
    assert (y.n_freq, y.F1, y.F2, y.rnn_input_size) == (161, 81, 41, 1312)
    for cfg, mm in ((C.SMALL, m), (C.YAML_GEOMETRY, y)):
        assert {k: tuple(v.shape) for k, v in mm.state_dict().items()} == C.param_shapes(**cfg)


def test_signature_refusals():
    from mindaudio_amd.models import DeepSpeechModel

    conf = dict(sample_rate=1600, window_size=0.02)
    with pytest.raises(NotImplementedError):
        DeepSpeechModel(1, C.LABELS, 64, 1, conf, rnn_type="GRU")
    with pytest.raises(NotImplementedError):
        DeepSpeechModel(1, C.LABELS, 64, 1, conf, bidirectional=False)
    with pytest.raises(NotImplementedError):
        DeepSpeechModel(1, C.LABELS, 96, 1, conf)


def test_batchnorm_fold():
    from mindaudio_amd.models.deepspeech2 import fold_batchnorm

    g = np.random.RandomState(0)
    p = {"bn.gamma": g.uniform(0.5, 2, 32), "bn.beta": g.normal(0, 1, 32), "bn.moving_mean": g.normal(0, 1, 32),
         "bn.moving_variance": g.uniform(0.1, 3, 32)}
    x = g.normal(0, 2, (2, 32, 5, 7))
    scale, shift = fold_batchnorm(p["bn.gamma"], p["bn.beta"], p["bn.moving_mean"], p["bn.moving_variance"])
    assert scale.dtype == shift.dtype == np.float32
    got = x * scale[None, :, None, None].astype(np.float64) + shift[None, :, None, None].astype(np.float64)
    want = C.batchnorm(x, p, "bn.")
    assert np.abs(got - want).max() <= 2.0 ** -23 * (np.abs(want).max() + np.abs(x).max() * np.abs(scale).max())


def test_wih_column_permutation():
    from mindaudio_amd.models.deepspeech2 import permute_wih_columns

    F2, H4 = 5, 8
    w = np.arange(H4 * 32 * F2, dtype=np.float32).reshape(H4, 32 * F2)
    got = permute_wih_columns(torch.from_numpy(w), 32, F2).numpy()
    for c in (0, 3, 31):
        for f in (0, 2, 4):
            assert np.array_equal(got[:, f * 32 + c], w[:, c * F2 + f])
    # the product on permuted features equals the reference's product on its own order
    y = np.random.RandomState(1).normal(0, 1, (2, 32, F2, 3))
    ref_in = C.rnn_input(y)                                        # feature c * F2 + f
    own_in = y.transpose(3, 0, 2, 1).reshape(3, 2, F2 * 32)        # feature f * 32 + c
    assert np.allclose(ref_in @ w.T.astype(np.float64), own_in @ got.T.astype(np.float64), rtol=0, atol=1e-6)


def test_checkpoint_names_round_trip(tmp_path):
    from mindaudio_amd.utils import ckpt

    m = _model(C.SMALL)
    state = C.make_state(C.SMALL, 5)
    m.load_weights(state)
    ref = ckpt.deepspeech2_to_reference_names(m.state_dict())
    assert sorted(ref) == sorted(C.param_shapes(**C.SMALL))
    extra = dict(ref)
    extra["moments.conv.conv1.weight"] = np.zeros((32, 1, 41, 11), np.float32)  # optimizer state is dropped
    extra["conv.module_list.0.weight"] = ref["conv.conv1.weight"]                # MaskConv's second registration is ignored
    path = str(tmp_path / "ds2.ckpt")
    ckpt.write_mindspore_ckpt(path, extra)
    m2 = _model(C.SMALL)
    missing, unexpected = m2.load_checkpoint(path)
    assert missing == [] and unexpected == []
    for k, v in m2.state_dict().items():
        assert np.array_equal(v.numpy(), state[k]), k
    with pytest.raises(KeyError):
        m2.load_weights({k: v for k, v in state.items() if k != "fc.module.weight"})


def test_forward_without_gpu_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mindaudio_amd._lib import MindaudioAmdError

    m = _model(C.SMALL)
    with pytest.raises(MindaudioAmdError):
        m(C.make_input(C.SMALL, 0), np.array([45, 45, 45], np.int32))


# ---- decoder and error rates ----------------------------------------------------------------------------------------------------------------
def _ids(s):
    return [C.LABELS.index(ch) for ch in s]


DECODE_CASES = [  # (frames, size, expected) by hand from process_string
    ("A_A", 3, "AA"),          # a blank between two equal characters keeps both
    ("AA", 2, "A"),            # equal neighbours collapse
    ("A___B", 5, "AB"),        # a blank run
    ("HI_ _YOU", 8, "HI YOU"),  # the space label
    ("ABCD", 2, "AB"),         # size shorter than T
    ("____", 4, ""),           # all blank
    ("AAB_BBA", 7, "ABBA"),
]


def test_greedy_decoder_by_hand():
    from mindaudio_amd.models.decoders import MSGreedyDecoder

    dec = MSGreedyDecoder(C.LABELS, blank_index=C.LABELS.index("_"))
    T = max(len(f) for f, _, _ in DECODE_CASES)
    probs = np.full((len(DECODE_CASES), T, len(C.LABELS)), 0.01, np.float32)
    sizes = []
    for b, (frames, size, want) in enumerate(DECODE_CASES):
        ids = _ids(frames) + [C.LABELS.index("_")] * (T - len(frames))
        probs[b, np.arange(T), ids] = 0.7
        sizes.append(size)
        assert dec.process_string(np.array(ids), size, remove_repetitions=True)[0] == want
        assert C.greedy_string(ids, size) == want
    strings, offsets = dec.decode(probs, np.array(sizes, np.int32))
    assert [s[0] for s in strings] == [w for _, _, w in DECODE_CASES]
    assert offsets[0][0] == [0, 2] and offsets[3][0] == [0, 1, 3, 5, 6, 7]
    assert dec.convert_to_strings([_ids("A A")])[0][0] == "A A"  # targets: no repetition removal


def test_error_counts_by_hand():
    from mindaudio_amd.models.decoders import MSGreedyDecoder

    dec = MSGreedyDecoder(C.LABELS, blank_index=C.LABELS.index("_"))
    # (hypothesis, reference, word edits, character edits without spaces)
    for hyp, ref, w, c in [("THE CAT SAT", "THE CAT SAT", 0, 0),
                           ("THE CAT SAT", "THE BAT SAT DOWN", 2, 5),   # CAT -> BAT, + DOWN | C -> B, + D O W N
                           ("HELLOWORLD", "HELLO WORLD", 2, 0)]:        # one word against two: substitute + insert | same letters
        assert dec.wer(hyp, ref) == w and dec.cer(hyp, ref) == c


def test_split_targets():
    from mindaudio_amd.deepspeech2.eval import split_targets

    idx = np.array([[0, 0], [0, 1], [1, 0], [2, 0], [2, 1], [2, 2]], np.int64)
    assert split_targets(idx, np.array([5, 6, 7, 8, 9, 10], np.int32)) == [[5, 6], [7], [8, 9, 10]]


# ---- dataset ----------------------------------------------------------------------------------------------------------------------------
def test_asr_dataset_eval_batching(tmp_path):
    from oracle.speech_features import read_wav

    from mindaudio_amd.deepspeech2.dataset import TEST_INPUT_PAD_LENGTH, ASRDataset

    wave, _ = read_wav(C.WAV)
    texts = ["HI YOU", "A'B", "CAB", "", "ZED Q"]
    samples = []
    for i, text in enumerate(texts):
        with open(tmp_path / ("t%d.txt" % i), "w") as fh:
            fh.write(text + "\n")
        samples.append({"wav_path": "w%d" % i, "transcript_path": "t%d.txt" % i})
    manifest = tmp_path / "manifest.json"
    manifest.write_text(json.dumps({"root_path": str(tmp_path), "samples": samples}))
    conf = dict(sample_rate=16000, window_size=0.02, window_stride=0.01)

    class HostDataset(ASRDataset):  # parse_audio answered by the NumPy restatement: the batching is what is under test
        def parse_audio(self, audio_path):
            n = 16000 + 1600 * int(os.path.basename(audio_path)[1:])
            return C.parse_audio(wave[:n], 16000, 0.02, 0.01, self.is_normalization)[0].astype(np.float32)

    ds = HostDataset(conf, str(manifest), C.LABELS, normalize=True, batch_size=2)
    assert len(ds) == 3 and [len(b) for b in ds.bins] == [2, 2, 2]
    assert [s[0] for s in ds.bins[2]] == ["w3", "w4"]  # the last bin is refilled from the tail
    inputs, input_length, target_indices, targets = ds[0]
    assert inputs.shape == (2, 1, 161, TEST_INPUT_PAD_LENGTH) and inputs.dtype == np.float32
    assert input_length.dtype == np.float32 and input_length.tolist() == [101.0, 111.0]
    assert np.all(inputs[0, 0, :, 101:] == 0) and np.all(inputs[1, 0, :, 111:] == 0) and np.abs(inputs[0, 0, :, 100]).max() > 0
    want0 = [C.LABELS.index(ch) for ch in "HI YOU"]
    want1 = [C.LABELS.index(ch) for ch in "AB"]  # label 0 (the apostrophe) is dropped by the reference's filter(None, ...)
    assert targets.dtype == np.int32 and targets.tolist() == want0 + want1
    assert target_indices.dtype == np.int64
    assert target_indices.tolist() == [[0, m] for m in range(6)] + [[1, m] for m in range(2)]
    _, _, idx2, t2 = ds[2]
    assert idx2.shape == (5, 2) and idx2[:, 0].tolist() == [1] * 5 and len(t2) == 5  # an empty transcript contributes nothing
    with pytest.raises(NotImplementedError):
        ASRDataset(conf, str(manifest), C.LABELS, is_training=True)
