"""examples/wavegrad/dataset.py without MindSpore: the manifest, the `_wav.npy` / `_feature.npy` pairs that preprocess.py writes, and
the batch map that crops and diffuses every utterance.

Kept from the reference: np.random is the one generator, in the reference's call order - per utterance the crop start
`randint(0, frames - crop_mel_frames)` (exclusive: the last possible start is never drawn, and an utterance of exactly
crop_mel_frames frames raises), then diffuse's `randint(1, S + 1)`, `rand()`, `randn(*x.shape)`; the manifest is shuffled under
`np.random.seed(0)` and split 99 : 1 (ljspeech.py:70-79).  Not built: the LJSpeech download / manifest creation (ljspeech.py:29-61)
and the sampler's per-epoch shuffle - the training split is walked in its (shuffled once) order."""
import numpy as np

FEATURE_POSTFIX = "_feature.npy"
WAV_POSTFIX = "_wav.npy"


def noise_levels(hps):
    """dataset.py:44-49: sqrt(cumprod(1 - beta)) behind a leading 1, float32, S + 1 values."""
    beta = np.linspace(hps.noise_schedule_start, hps.noise_schedule_end, hps.noise_schedule_S)
    return np.concatenate([[1.0], np.cumprod(1 - beta) ** 0.5], axis=0).astype(np.float32)


def diffuse(x, S, noise_level):
    """One training pair of dataset.py:10-18: a step s in 1 .. S, a noise scale drawn uniformly between the levels of s - 1 and s,
    Gaussian noise -> (noisy_audio = scale x + sqrt(1 - scale^2) noise as float32, the scale as a float32 scalar, the noise as float32).
    Draw order: randint, rand, randn."""
    step = np.random.randint(1, S + 1)
    below, above = noise_level[step - 1], noise_level[step]
    fraction = np.random.rand()
    scale = (below + fraction * (above - below)).astype(np.float32)
    noise = np.random.randn(*x.shape).astype(np.float32)
    mixed = scale * x + (1.0 - scale ** 2) ** 0.5 * noise
    return mixed.astype(np.float32), scale, noise


def batch_collate(audio, spectrogram, hps, noise_level):
    """The per-batch map of dataset.py:53-85.  audio: waveforms (n,); spectrogram: features (n_mels, frames).  Every utterance is cut
    to crop_mel_frames frames at a random start (the waveform to the matching crop * hop samples, zero-padded at its end), then
    diffused -> (noisy_audio (B, crop * hop), noise_scale (B,), noise (B, crop * hop), spectrogram (B, n_mels, crop))."""
    hop, crop = hps.hop_samples, hps.crop_mel_frames
    rows = []
    for wave, mel in zip(audio, spectrogram):
        first = np.random.randint(0, mel.shape[1] - crop)
        piece = wave[first * hop:(first + crop) * hop]
        piece = np.pad(piece, (0, crop * hop - len(piece)), mode="constant")
        rows.append(diffuse(piece, hps.noise_schedule_S, noise_level) + (mel[:, first:first + crop],))
    return tuple(np.stack([row[i] for row in rows]) for i in range(4))


def read_manifest(manifest_path, is_train=True):
    """The wav paths of a tab-separated manifest (wav path, text path), shuffled under seed 0 and split as ljspeech.py:63-79 does."""
    bins = []
    with open(manifest_path) as f:
        for line in f:
            if line.strip():
                bins.append(line.strip().split("\t")[0])
    np.random.seed(0)
    np.random.shuffle(bins)
    cut = int(0.99 * len(bins))
    return bins[:cut] if is_train else bins[cut:]


def read_pair(wav_path):
    """dataset.py:29-33: the waveform and the feature that preprocess.py saved beside `wav_path`."""
    return np.load(wav_path.replace(".wav", WAV_POSTFIX)), np.load(wav_path.replace(".wav", FEATURE_POSTFIX))


class WaveGradDataset:
    """create_wavegrad_dataset(hps, batch_size, is_train): len() = whole batches per epoch (drop_remainder); iterating yields the four
    arrays of batch_collate, batch after batch in the split's order."""

    def __init__(self, hps, batch_size, is_train=True):
        self.hps, self.batch_size = hps, int(batch_size)
        self.paths = read_manifest(hps.manifest_path, is_train)
        self.noise_level = noise_levels(hps)
        if self.batch_size < 1:
            raise ValueError("batch_size must be positive")

    def __len__(self):
        return len(self.paths) // self.batch_size

    def __iter__(self):
        for i in range(len(self)):
            pairs = [read_pair(p) for p in self.paths[i * self.batch_size:(i + 1) * self.batch_size]]
            yield batch_collate([p[0] for p in pairs], [p[1] for p in pairs], self.hps, self.noise_level)
