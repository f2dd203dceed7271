"""examples/deepspeech2/dataset.py: LoadAudioAndTranscript.parse_audio on the device and ASRDataset's batching, evaluation and training.

parse_audio: stft(n_fft = win_length = sample_rate * window_size, hop = sample_rate * window_stride) with stft's DEFAULT window - the
yaml's `window: "hamming"` is never passed on by the reference (dataset.py:39-41) - then magphase(power = 1), log1p and, with
`normalize`, (mag - mag.mean()) / mag.std() over the whole utterance's spectrogram (population standard deviation; the statistics
are float64, as data.processing.normalize computes them).

ASRDataset (is_training=False): the manifest json {"root_path": ..., "samples": [{"wav_path": ..., "transcript_path": ...}, ...]},
bins of batch_size utterances with the last bin refilled from the tail of the list (dataset.py:88-91), every utterance zero-padded to
TEST_INPUT_PAD_LENGTH = 3500 frames, input_length (float32, as the reference returns it), target_indices (n, 2) int64 and the flat
label_values int32.

ASRTrainDataset (ASRDataset(is_training=True) itself still refuses, as it always has): the same bins, the refilled last one
included, every utterance zero-padded to TRAIN_INPUT_PAD_LENGTH = 1250 frames; a longer one is cropped to 1250 frames from a start drawn with np.random.randint(seq_length - 1250), one draw per long
utterance in batch order - the reference's draws under the same NumPy seed.  Where the reference pads every target row to 350 entries
with the blank id and hands all 350 to the loss as labels, this returns targets (b, Lmax) int32 (blank-padded) WITH the true
target_lengths (b,) int32.  Utterances whose transcript has more than MAX_TARGET_LENGTH = 223 labels (the limit of
ma_ctc_loss_grad_f32) are dropped from the list before it is cut into bins, with one printed count.
The MindSpore GeneratorDataset wrapper (DistributedSampler, shuffling) is not built."""
import json
import os

import numpy as np

TEST_INPUT_PAD_LENGTH = 3500  # the max length in the test dataset (LibriSpeech), dataset.py:15
TRAIN_INPUT_PAD_LENGTH = 1250  # dataset.py:11
MAX_TARGET_LENGTH = 223  # labels per utterance that ma_ctc_loss_grad_f32 takes


def _conf(audio_conf, key):
    return audio_conf[key] if isinstance(audio_conf, dict) else getattr(audio_conf, key)


class LoadAudioAndTranscript:
    def __init__(self, audio_conf=None, normalize=False, labels=None):
        self.window_stride = _conf(audio_conf, "window_stride")
        self.window_size = _conf(audio_conf, "window_size")
        self.sample_rate = _conf(audio_conf, "sample_rate")
        self.is_normalization = normalize
        self.labels = labels

    def spectrogram(self, audio):
        """A waveform (NumPy or device tensor) -> the (n_fft / 2 + 1, frames) float32 device tensor of parse_audio."""
        from .. import _host
        from ..data import processing, spectrum

        t = _host.require_gpu()
        n_fft = int(self.sample_rate * self.window_size)
        hop_length = int(self.sample_rate * self.window_stride)
        if not isinstance(audio, t.Tensor):
            audio = t.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).cuda()
        spec = spectrum.stft(audio, n_fft=n_fft, hop_length=hop_length, win_length=n_fft)
        mag, _ = spectrum.magphase(spec, power=1.0, iscomplex=True)
        mag = t.log1p(mag).contiguous()
        if self.is_normalization:
            mean = processing.axis_stats_device(mag, None, _lib_const("AXIS_MEAN"))
            std = processing.axis_stats_device(mag, None, _lib_const("AXIS_STD"))
            mag = processing.axis_apply_device(mag, None, sub=mean, div=std)
        return mag

    def parse_audio(self, audio_path):
        from ..data.io import read

        audio, _ = read(str(audio_path))
        return self.spectrogram(audio)

    def parse_transcript(self, transcript_path):
        with open(transcript_path, "r", encoding="utf8") as transcript_file:
            transcript = transcript_file.read().replace("\n", "")
        return [i for i in (self.labels.get(x) for x in list(transcript)) if i]  # (filter(None, ...): label 0 is dropped too)


def _lib_const(name):
    from .. import _lib

    return getattr(_lib, name)


class ASRDataset(LoadAudioAndTranscript):
    def __init__(self, audio_conf=None, manifest_filepath="", labels=None, normalize=False, batch_size=32, is_training=False):
        if is_training != isinstance(self, ASRTrainDataset):
            raise NotImplementedError("ASRDataset is the evaluation data set; the training one is ASRTrainDataset")
        with open(manifest_filepath) as f:
            json_file = json.load(f)
        self.root_path = json_file.get("root_path")
        self.labels_map = {labels[i]: i for i in range(len(labels))}
        super().__init__(audio_conf, normalize, self.labels_map)
        ids = self._select([list(x.values()) for x in json_file.get("samples")])
        self.is_training = is_training
        self.ids = ids
        self.blank_id = int(labels.index("_"))
        self.bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]
        if len(self.ids) % batch_size != 0:
            self.bins = self.bins[:-1]
            self.bins.append(ids[-batch_size:])
        self.size = len(self.bins)
        self.batch_size = batch_size

    def _select(self, ids):
        return ids

    def _load(self, index):
        if index >= self.size:
            raise IndexError(index)
        batch_spect, batch_script = [], []
        for data in self.bins[index]:
            batch_spect.append(self.parse_audio(os.path.join(self.root_path, data[0])))
            batch_script.append(self.parse_transcript(os.path.join(self.root_path, data[1])))
        return batch_spect, batch_script

    @staticmethod
    def _zeros(like, shape):
        if isinstance(like, np.ndarray):  # (a parse_audio that answers in NumPy is batched in NumPy)
            return np.zeros(shape, dtype=np.float32)
        return like.new_zeros(shape)

    def __getitem__(self, index):
        """(inputs (b, 1, F, 3500) float32 device tensor, input_length (b,) float32, target_indices (n, 2) int64, targets (n,) int32)"""
        batch_spect, batch_script = self._load(index)
        batch_size, target_indices, targets = len(batch_spect), [], []
        input_length = np.zeros(batch_size, np.float32)
        inputs = self._zeros(batch_spect[-1], (batch_size, 1, batch_spect[-1].shape[0], TEST_INPUT_PAD_LENGTH))
        for k, (spect_, scripts_) in enumerate(zip(batch_spect, batch_script)):
            seq_length = spect_.shape[1]
            input_length[k] = seq_length
            targets.extend(scripts_)
            target_indices.extend([k, m] for m in range(len(scripts_)))
            inputs[k, 0, :, 0:seq_length] = spect_  # (longer than 3500 frames: the same shape error as the reference's assignment)
        return inputs, input_length, np.array(target_indices, dtype=np.int64).reshape(-1, 2), np.array(targets, dtype=np.int32)

    def __len__(self):
        return self.size


class ASRTrainDataset(ASRDataset):
    """ASRDataset's training branch (dataset.py:113-145); `log` receives the one line that counts the dropped utterances."""

    def __init__(self, audio_conf=None, manifest_filepath="", labels=None, normalize=False, batch_size=32, log=print):
        self.log, self.dropped = log, 0
        super().__init__(audio_conf, manifest_filepath, labels, normalize, batch_size, is_training=True)

    def _select(self, ids):
        kept = [x for x in ids if len(self.parse_transcript(os.path.join(self.root_path, x[1]))) <= MAX_TARGET_LENGTH]
        self.dropped = len(ids) - len(kept)
        if self.dropped:
            self.log("dropped %d of %d utterances: more than %d labels" % (self.dropped, len(ids), MAX_TARGET_LENGTH))
        if not kept:
            raise ValueError("no utterance to train on")
        return kept

    def __getitem__(self, index):
        """(inputs (b, 1, F, 1250) float32, input_length (b,) float32, targets (b, Lmax) int32 padded with the blank id, target_lengths
        (b,) int32)"""
        batch_spect, batch_script = self._load(index)
        b = len(batch_spect)
        inputs = self._zeros(batch_spect[-1], (b, 1, batch_spect[-1].shape[0], TRAIN_INPUT_PAD_LENGTH))
        input_length = np.zeros(b, np.float32)
        target_lengths = np.array([len(s) for s in batch_script], np.int32)
        targets = np.full((b, max(1, int(target_lengths.max()))), self.blank_id, np.int32)
        for k, (spect_, scripts_) in enumerate(zip(batch_spect, batch_script)):
            seq_length = spect_.shape[1]
            targets[k, :len(scripts_)] = scripts_
            if seq_length <= TRAIN_INPUT_PAD_LENGTH:
                input_length[k] = seq_length
                inputs[k, 0, :, 0:seq_length] = spect_
            else:  # a random crop; one draw per long utterance, in batch order
                start = np.random.randint(seq_length - TRAIN_INPUT_PAD_LENGTH)
                input_length[k] = TRAIN_INPUT_PAD_LENGTH
                inputs[k, 0] = spect_[:, start:start + TRAIN_INPUT_PAD_LENGTH]
        return inputs, input_length, targets, target_lengths
