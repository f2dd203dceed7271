"""The feature side of examples/wavegrad/preprocess.py: read_wav, _normalize and the spectrogram -> mel -> _normalize chain of
reverse.py:53-82 as `mel_features`.  The dataset dump (create_prep_dataset, preprocess_ljspeech) and ljspeech.py are not built."""
import numpy as np


def read_wav(filename):
    """preprocess.py:17-24: int16 samples / 32768, then peak-normalised.  -> (audio, audio, filename) as the reference returns."""
    from ..data.io import read

    filename = str(filename).replace("b'", "").replace("'", "")
    audio, _ = read(filename)
    if audio.dtype == np.int16:
        audio = audio.astype(np.float32) / 2 ** 15
    audio = audio / np.max(np.abs(audio))
    return audio, audio, filename


def _normalize(S):
    """preprocess.py:27-30, NumPy in, NumPy out: clip((20 log10(clip(S, 1e-5)) - 20 + 100) / 100, 0, 1) as float32."""
    S = 20 * np.log10(np.clip(S, 1e-5, None)) - 20
    S = np.clip((S + 100) / 100, 0.0, 1.0)
    return S.astype(np.float32)


def mel_spectrum(wav, hps):
    """The magnitude mel spectrum before _normalize: (n_mels, frames) float32 on the device.  Spectrogram(n_fft, win_length = 4 hop,
    hop, power 1, centred, reflect) through data.spectrum.spectrogram (the power-of-two FFT path), times the HTK bank
    MelScale(n_mels, sample_rate, f_min 20, f_max sample_rate / 2, n_stft n_fft // 2 + 1)."""
    import torch

    from .. import _host
    from ..data.spectrum import spectrogram

    t = _host.require_gpu()
    x = torch.as_tensor(np.asarray(wav, dtype=np.float32)) if not isinstance(wav, t.Tensor) else wav.to(torch.float32)
    spec = spectrogram(x.cuda(), n_fft=hps.n_fft, win_length=hps.hop_samples * 4, hop_length=hps.hop_samples, power=1.0, center=True,
                       pad_mode="reflect")
    bank = _host.mel_fbanks_f64(hps.n_fft // 2 + 1, 20.0, hps.sample_rate / 2.0, hps.n_mels, hps.sample_rate)
    # once per utterance on an (n_mels, frames) array: plain tensor ops
    return torch.matmul(torch.from_numpy(bank.T.astype(np.float32)).to(spec.device), spec)


def mel_features(wav, hps):
    """reverse.py:78-81 without the batch axis: _normalize(mel(stft(wav))) -> (n_mels, frames) float32 ndarray."""
    return _normalize(mel_spectrum(wav, hps).cpu().numpy())
