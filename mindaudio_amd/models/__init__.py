from .conformer import ConformerEncoder  # noqa: F401
from .conv_tasnet import ConvTasNet  # noqa: F401
from .deepspeech2 import DeepSpeechModel  # noqa: F401
from .ecapatdnn import EcapaTDNN  # noqa: F401
from .ecapatdnn import Classifier  # noqa: F401
from .fastspeech2 import FastSpeech2  # noqa: F401
from .tasnet import TasNet  # noqa: F401
from .wavegrad import WaveGrad  # noqa: F401
