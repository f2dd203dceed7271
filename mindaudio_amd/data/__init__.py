from .features import fbank, fbanks, harmonic, hpss, soft_mask  # noqa: F401
from .spectrum import amplitude_to_dB, frame, melspectrogram, stft  # noqa: F401
