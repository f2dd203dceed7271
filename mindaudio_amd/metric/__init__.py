"""Host-side metrics next to the hot path (mirror of mindaudio/metric)."""
from .eer import EER, compute_fa_miss, get_eer, get_eer_from_scores  # noqa: F401
from .snr import cal_SISNR, cal_SISNRi  # noqa: F401
from .wer import wer  # noqa: F401
