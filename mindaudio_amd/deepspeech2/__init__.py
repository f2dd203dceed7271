"""The DeepSpeech2 example (examples/deepspeech2): the evaluation data pipeline and `eval`.  Training and `librispeech_prepare` are not
built."""
from .dataset import ASRDataset, LoadAudioAndTranscript  # noqa: F401
