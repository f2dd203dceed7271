"""CPU: what surrounds the DeepSpeech2 training step - ASRTrainDataset's batching against a NumPy restatement of
examples/deepspeech2/dataset.py's training branch under a seed, the dropping of over-long transcripts, the yaml keys the script
reads, and its checkpoint names and rotation on a stub trainer."""
import json
import os

import numpy as np
import pytest
import torch

import deepspeech2_cases as C

YAML = """
TrainingConfig:
    epochs: 70
    batch_size: 64
    train_manifest: './train/libri_train_manifest.json'
SpectConfig:
    sample_rate: 16000
    window_size: 0.02
    window_stride: 0.01
    window: "hamming"
ModelConfig:
    rnn_type: "LSTM"
    hidden_size: 1024
    hidden_layers: 5
    lookahead_context: 20
OptimConfig:
    learning_rate: 0.0003
    learning_anneal: 1.1
    weight_decay: 0.00001
    momentum: 0.9
    eps: 0.000000001
    betas: (0.9, 0.999)
    loss_scale: 1024
    epsilon: 0.00001
CheckpointConfig:
    ckpt_file_name_prefix: 'DeepSpeech'
    ckpt_path: './checkpoint'
    keep_checkpoint_max: 10
Pretrained_model: ''
labels: ["'", "A", "B", "C", "D", "E", "F", "G", "H", "I", "J", "K", "L", "M",
         "N", "O", "P", "Q", "R", "S", "T", "U", "V", "W", "X", "Y", "Z", " ", "_"]
"""

FRAMES = [300, 1400, 1250, 2000, 1251]  # frames per utterance: short, long, exactly the pad, long, one over
TEXTS = ["HI YOU", "A'B", "", "CAB", "ZED Q"]


def _manifest(tmp_path, texts):
    samples = []
    for i, text in enumerate(texts):
        with open(tmp_path / ("t%d.txt" % i), "w") as fh:
            fh.write(text + "\n")
        samples.append({"wav_path": "w%d" % i, "transcript_path": "t%d.txt" % i})
    path = tmp_path / "manifest.json"
    path.write_text(json.dumps({"root_path": str(tmp_path), "samples": samples}))
    return str(path)


def _spect(i, F=9):
    """A (F, FRAMES[i]) spectrogram whose value names its utterance and frame."""
    return (1000.0 * (i + 1) + np.arange(FRAMES[i], dtype=np.float32))[None, :] + 0.001 * np.arange(F, dtype=np.float32)[:, None]


def _host_dataset(manifest, batch_size, log=print):
    from mindaudio_amd.deepspeech2.dataset import ASRTrainDataset

    class HostDataset(ASRTrainDataset):  # parse_audio answered in NumPy: the batching is what is under test
        def parse_audio(self, audio_path):
            return _spect(int(os.path.basename(audio_path)[1:]))

    return HostDataset(dict(sample_rate=16000, window_size=0.02, window_stride=0.01), manifest, C.LABELS, normalize=True,
                       batch_size=batch_size, log=log)


def test_training_batching_against_numpy(tmp_path):
    from mindaudio_amd.deepspeech2.dataset import TRAIN_INPUT_PAD_LENGTH

    assert TRAIN_INPUT_PAD_LENGTH == 1250
    ds = _host_dataset(_manifest(tmp_path, TEXTS), 2)
    assert len(ds) == 3 and [[s[0] for s in b] for b in ds.bins] == [["w0", "w1"], ["w2", "w3"], ["w3", "w4"]]  # the refilled last bin
    np.random.seed(5)
    got = [ds[i] for i in range(3)]
    # the restatement: one np.random.randint(seq_length - 1250) per utterance longer than 1250 frames, in batch order, bins in order
    np.random.seed(5)
    for (inputs, input_length, targets, target_lengths), members in zip(got, ([0, 1], [2, 3], [3, 4])):
        assert inputs.shape == (2, 1, 9, 1250) and inputs.dtype == np.float32 and input_length.dtype == np.float32
        labels = [[C.LABELS.index(ch) for ch in TEXTS[i] if C.LABELS.index(ch)] for i in members]  # label 0 is dropped: filter(None, ...)
        assert target_lengths.dtype == np.int32 and target_lengths.tolist() == [len(v) for v in labels]
        assert targets.dtype == np.int32 and targets.shape == (2, max(1, max(len(v) for v in labels)))
        for k, i in enumerate(members):
            want = np.zeros((9, 1250), np.float32)
            if FRAMES[i] <= 1250:
                want[:, :FRAMES[i]] = _spect(i)
                assert input_length[k] == FRAMES[i]
            else:
                start = np.random.randint(FRAMES[i] - 1250)
                want[:] = _spect(i)[:, start:start + 1250]
                assert input_length[k] == 1250
            assert np.array_equal(inputs[k, 0], want)
            assert targets[k].tolist() == labels[k] + [28] * (targets.shape[1] - len(labels[k]))  # padded with the blank id


def test_eval_class_still_refuses_training(tmp_path):
    from mindaudio_amd.deepspeech2.dataset import ASRDataset

    manifest = _manifest(tmp_path, TEXTS)
    with pytest.raises(NotImplementedError):
        ASRDataset(dict(sample_rate=16000, window_size=0.02, window_stride=0.01), manifest, C.LABELS, is_training=True)


def test_over_long_transcripts_are_dropped_with_one_count(tmp_path):
    texts = ["AB", "A" * 224, "C" * 223, "B" * 300, "HI"]
    lines = []
    ds = _host_dataset(_manifest(tmp_path, texts), 2, log=lines.append)
    assert lines == ["dropped 2 of 5 utterances: more than 223 labels"] and ds.dropped == 2
    assert [s[0] for s in ds.ids] == ["w0", "w2", "w4"]
    assert [[s[0] for s in b] for b in ds.bins] == [["w0", "w2"], ["w2", "w4"]]
    lines.clear()
    assert _host_dataset(_manifest(tmp_path, ["AB", "HI"]), 2, log=lines.append).dropped == 0 and lines == []
    with pytest.raises(ValueError):
        _host_dataset(_manifest(tmp_path, ["A" * 224]), 2, log=lines.append)


def test_script_reads_the_yaml(tmp_path):
    from mindaudio_amd.conformer.train import load_config
    from mindaudio_amd.deepspeech2 import train as T

    path = tmp_path / "deepspeech2.yaml"
    path.write_text(YAML)
    s = T.settings(load_config(str(path), {"Pretrained_model": None}))
    assert (s["epochs"], s["batch_size"], s["hidden_size"], s["hidden_layers"], s["rnn_type"]) == (70, 64, 1024, 5, "LSTM")
    assert (s["learning_rate"], s["epsilon"], s["optimizer_loss_scale"]) == (0.0003, 1e-5, 1024.0)  # epsilon, not eps, is Adam's
    assert (s["prefix"], s["ckpt_path"], s["keep_checkpoint_max"], s["pretrained"]) == ("DeepSpeech", "./checkpoint", 10, "")
    assert s["labels"] == C.LABELS and s["labels"].index("_") == 28
    assert T.SAVE_CHECKPOINT_STEPS == 5 and T.LOSS_SCALE == 1024
    assert T.settings(load_config(str(path), {"Pretrained_model": "x.ckpt"}))["pretrained"] == "x.ckpt"
    with pytest.raises(NotImplementedError):
        T.train(load_config(str(path)), is_distributed=True)
    with pytest.raises(SystemExit):
        T.main([])  # --config_path is required


def test_checkpoint_names_and_rotation(tmp_path):
    from mindaudio_amd.deepspeech2.train import Checkpoints
    from mindaudio_amd.utils import ckpt

    class StubTrainer:
        step = 0

        def state_dict(self):
            return {"fc.module.weight": torch.full((2, 3), float(self.step)), "moment1.fc.module.weight": torch.zeros(2, 3),
                    "steps": torch.tensor(self.step)}

    tr = StubTrainer()
    saver = Checkpoints(tr, str(tmp_path / "ck"), "DeepSpeech", keep_max=2)
    steps_per_epoch, written = 7, []
    for g in range(1, 22):  # three epochs of 7 steps
        tr.step = g
        path = saver.after_step(g, (g - 1) // steps_per_epoch + 1, (g - 1) % steps_per_epoch + 1)
        assert (path is not None) == (g % 5 == 0)
        if path:
            written.append(os.path.basename(path))
    assert written == ["DeepSpeech-1_5.ckpt", "DeepSpeech-2_3.ckpt", "DeepSpeech-3_1.ckpt", "DeepSpeech-3_6.ckpt"]
    assert sorted(os.listdir(tmp_path / "ck")) == ["DeepSpeech-3_1.ckpt", "DeepSpeech-3_6.ckpt"]  # keep_checkpoint_max = 2
    raw = ckpt.read_mindspore_ckpt(str(tmp_path / "ck" / "DeepSpeech-3_6.ckpt"))
    assert sorted(raw) == ["fc.module.weight", "global_step", "moment1.fc.module.weight"] and int(raw["global_step"][0]) == 20 and np.all(np.asarray(raw["fc.module.weight"]) == 20.0)
