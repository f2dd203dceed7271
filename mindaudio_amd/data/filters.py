"""mindaudio.data.filters.notch_filter (filters.py:24-76): a host function - 101 float64 numbers per call, composed into the drop
filter of augment.drop_freq on the host and applied on the device.  The IIR filters of filters.py are not built."""
import numpy as np

__all__ = ["notch_filter"]


def notch_filter(notch_freq, filter_width=101, notch_width=0.05):
    """(1, filter_width, 1) float64 notch kernel: a low-pass below and a high-pass above `notch_freq` (a fraction of the Nyquist
    rate), Blackman-windowed sincs with the reference's constants (cutoff factor 3, `np.blackman(width + 1)[:-1]`)."""
    assert filter_width % 2 != 0
    assert 0 < notch_freq <= 1
    pad = filter_width // 2
    notch_freq += notch_width
    inputs = np.arange(filter_width) - pad

    def sinc(x):  # the zero is at the middle index
        return np.concatenate([np.sin(x[:pad]) / x[:pad], np.ones(1), np.sin(x[pad + 1:]) / x[pad + 1:]])

    window = np.blackman(filter_width + 1)[:-1]
    hlpf = sinc(3 * (notch_freq - notch_width) * inputs)
    hlpf *= window
    hlpf /= np.sum(hlpf)
    hhpf = sinc(3 * (notch_freq + notch_width) * inputs)
    hhpf *= window
    hhpf /= -np.sum(hhpf)
    hhpf[pad] += 1
    return (hlpf + hhpf).reshape(1, -1, 1)
