"""Scale-invariant SNR metrics with the call signatures of mindaudio/metric/snr.py, on the host in float64 whatever the input type.
`cal_SDRi` needs mir_eval.separation.bss_eval_sources, which this package does not depend on: it is not built."""
import numpy as np

__all__ = ["cal_SISNR", "cal_SISNRi"]


def _si_snr_db(target, signal, eps):
    """10 log10(|p|^2 / (|signal - p|^2 + eps) + eps) for zero-mean float64 vectors, p = the projection of `signal` on `target`
    with eps added to the target's energy - the three places the reference puts its eps."""
    p = target * (np.dot(target, signal) / (np.dot(target, target) + eps))
    residual = signal - p
    return 10.0 * np.log(np.dot(p, p) / (np.dot(residual, residual) + eps) + eps) / np.log(10.0)


def _centred(x):
    x = np.asarray(x, dtype=np.float64)
    return x - x.mean()


def cal_SISNR(ref_sig, out_sig, eps=1e-8):
    """SI-SNR in dB of the estimate `out_sig` against the reference `ref_sig`, both (T,)."""
    if len(ref_sig) != len(out_sig):
        raise ValueError("cal_SISNR: the two signals differ in length")
    return _si_snr_db(_centred(ref_sig), _centred(out_sig), eps)


def cal_SISNRi(src_ref, src_est, mix):
    """Mean over the two sources of SI-SNR(reference, estimate) - SI-SNR(reference, mixture): src_ref, src_est (2, T), the
    estimate already in the references' order, mix (T,)."""
    gains = [cal_SISNR(src_ref[c], src_est[c]) - cal_SISNR(src_ref[c], mix) for c in range(2)]
    return sum(gains) / 2
