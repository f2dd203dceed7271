# (the loop and the script are mindaudio_amd.wavegrad.reverse: a function of that name here would hide the module)
from .config import Config, load_config  # noqa: F401
from .dataset import WaveGradDataset, batch_collate, diffuse  # noqa: F401
from .preprocess import _normalize, mel_features, read_wav  # noqa: F401
