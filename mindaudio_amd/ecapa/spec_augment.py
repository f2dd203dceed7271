"""examples/ECAPA-TDNN/spec_augment.py on the device: TimeDomainSpecAugment, EnvCorrupt, AddNoise, AddReverb, AddBabble and
InputNormalization with the example's constructor arguments and `construct(...)`.

`construct` takes NumPy (returns NumPy) or a device tensor (returns a device tensor), float32 `[batch, time]`.  With `out=` - a
(batch, n_out) float32 device view, for instance the augmenter's slice of the matrix the fbank reads - the last kernel of the chain
writes there, cut or zero-padded to n_out columns, and `out` is returned.  Random decisions are the host parts of data.augment: the
global `np.random` / `random` generators, in the reference's order.

What `construct` really does in the example is kept: TimeDomainSpecAugment calls speed_perturb(waves, sample_rate, speeds), then
drop_freq(waves) and drop_chunk(waves, lens) WITH THEIR DEFAULTS - the configured drop_* values are stored and never used; EnvCorrupt
applies reverb -> babble -> noise, each only if it was created.  Differences: the csv files are read with the `csv` module in file
order (the example reads them through a shuffling MindSpore CSVDataset whose order no seed of ours controls); `prepare_openrir`
downloads and is not here - `openrir_folder` is accepted when its noise.csv / reverb.csv already exist; AddNoise(normalize=True)
calls MindSpore ops on NumPy data in the example and is not built."""
import csv
import os

import numpy as np

from .. import _host, ops
from ..data import augment as A

__all__ = ["InputNormalization", "AddNoise", "AddReverb", "AddBabble", "EnvCorrupt", "TimeDomainSpecAugment"]


def _rows(waves):
    t = _host.require_gpu()
    was_numpy = not isinstance(waves, t.Tensor)
    if np.ndim(waves) != 2:
        raise NotImplementedError("construct takes [batch, time] waveforms")
    x = t.as_tensor(np.ascontiguousarray(waves) if was_numpy else waves).to(device="cuda", dtype=t.float32)
    return x, was_numpy


def _copy_rows(x, out):
    """x cut / zero-padded into out (a chain whose coins all said no still has to fill its slice)."""
    return ops.aug_drop_chunks(x, _host.torch().zeros((x.shape[0], 0, 2), dtype=_host.torch().int32), out=out)


def _finish(cur, x, out, was_numpy):
    if out is not None:
        return out if cur is out else _copy_rows(cur, out)
    if cur is x and not was_numpy:
        return x
    return cur.cpu().numpy() if was_numpy else cur


def _read_wav_column(csv_file):
    with open(csv_file, newline="") as fh:
        return [str(row["wav"]) for row in csv.DictReader(fh, skipinitialspace=True) if row.get("wav")]


class InputNormalization:
    """Sentence-level mean normalisation (the only way the example constructs it: norm_type="sentence", std_norm=False)."""

    def __init__(self, mean_norm=True, std_norm=True, norm_type="global"):
        if norm_type != "sentence" or std_norm or not mean_norm:
            raise NotImplementedError("only InputNormalization(norm_type='sentence', std_norm=False) is built")
        self.mean_norm, self.std_norm, self.norm_type, self.eps = mean_norm, std_norm, norm_type, 1e-10

    def construct(self, x_input):
        t = _host.require_gpu()
        was_numpy = not isinstance(x_input, t.Tensor)
        x = t.as_tensor(np.ascontiguousarray(x_input) if was_numpy else x_input).to(device="cuda", dtype=t.float32)
        y = ops.sentence_mean_norm(x)
        return y.cpu().numpy() if was_numpy else y


class AddNoise:
    """Adds one background row, cut from randomly chosen files of the csv's `wav` column, at one random SNR per batch."""

    def __init__(self, csv_file=None, csv_keys=None, sorting="random", num_workers=0, snr_low=0, snr_high=0, pad_noise=False,
                 mix_prob=1.0, start_index=None, normalize=False):
        if normalize:
            raise NotImplementedError("normalize=True is not built")
        self.csv_file, self.csv_keys, self.sorting, self.num_workers = csv_file, csv_keys, sorting, num_workers
        self.snr_low, self.snr_high, self.pad_noise, self.mix_prob = snr_low, snr_high, pad_noise, mix_prob
        self.start_index, self.normalize = start_index, normalize
        self.noise_data = _read_wav_column(csv_file)

    def _apply(self, x, out):
        dec = A.add_noise_host(x.shape[1], self.noise_data, self.snr_low, self.snr_high, self.mix_prob)
        if dec is None:
            return x
        return A.add_noise_device(x, A._dev(dec["background"], x.device, np.float32), dec["snr"], out=out)

    def construct(self, waveforms, out=None):
        x, was_numpy = _rows(waveforms)
        return _finish(self._apply(x, out), x, out, was_numpy)


class AddReverb:
    """Convolves the batch with one randomly chosen impulse response of the csv's `wav` column."""

    def __init__(self, csv_file, reverb_prob=1.0):
        self.csv_file, self.reverb_prob = csv_file, reverb_prob
        self.rir_data = _read_wav_column(csv_file)

    def _apply(self, x, out):
        dec = A.add_reverb_host(self.rir_data, self.reverb_prob)
        if dec is None:
            return x
        taps, rot = A.reverberate_host(dec["rir"], x.shape[1])
        return A.reverberate_device(x, taps, rot, out=out)

    def construct(self, waveforms, out=None):
        x, was_numpy = _rows(waveforms)
        return _finish(self._apply(x, out), x, out, was_numpy)


class AddBabble:
    """Mixes every row with the rows before it in the batch."""

    def __init__(self, speaker_count=3, snr_low=0, snr_high=0, mix_prob=1):
        self.speaker_count, self.snr_low, self.snr_high, self.mix_prob = speaker_count, snr_low, snr_high, mix_prob

    def _apply(self, x, lengths, out):
        dec = A.add_babble_host(lengths, x.shape[1], self.speaker_count, self.snr_low, self.snr_high, self.mix_prob)
        if dec is None:
            return x
        return A.add_babble_device(x, dec["params"], self.speaker_count, out=out)

    def construct(self, waveforms, lengths, out=None):
        x, was_numpy = _rows(waveforms)
        return _finish(self._apply(x, lengths, out), x, out, was_numpy)


class EnvCorrupt:
    """Environmental corruption: reverb, babble, noise - each applied when it was created."""

    def __init__(self, openrir_folder=None, openrir_max_noise_len=None, reverb_csv=None, noise_csv=None, reverb_prob=1.0,
                 babble_prob=1.0, noise_prob=1.0, noise_num_workers=0, noise_snr_low=0, noise_snr_high=0, babble_speaker_count=0,
                 babble_snr_low=0, babble_snr_high=0):
        if openrir_folder and (not noise_csv or not reverb_csv):
            open_noise_csv = os.path.join(openrir_folder, "noise.csv")
            open_reverb_csv = os.path.join(openrir_folder, "reverb.csv")
            for path in (open_noise_csv, open_reverb_csv):
                if not os.path.isfile(path):
                    raise FileNotFoundError("%s is missing: the example would download and unpack OpenRIR (rirs_noises.zip) here and "
                                            "write it; this port does not download - prepare the folder first" % path)
            noise_csv = noise_csv or open_noise_csv
            reverb_csv = reverb_csv or open_reverb_csv
        if noise_prob > 0.0 and noise_csv is not None:
            self.add_noise = AddNoise(csv_file=noise_csv, mix_prob=noise_prob, num_workers=noise_num_workers, snr_low=noise_snr_low,
                                      snr_high=noise_snr_high)
        if babble_prob > 0.0 and babble_speaker_count > 0:
            self.add_babble = AddBabble(mix_prob=babble_prob, speaker_count=babble_speaker_count, snr_low=babble_snr_low,
                                        snr_high=babble_snr_high)
        if reverb_prob > 0.0 and reverb_csv is not None:
            self.add_reverb = AddReverb(reverb_prob=reverb_prob, csv_file=reverb_csv)

    def construct(self, waves, lens, out=None):
        x, was_numpy = _rows(waves)
        cur = x
        # the first step that fires writes into `out`; the steps behind it work there in place (the mixes may alias their input)
        if hasattr(self, "add_reverb"):
            cur = self.add_reverb._apply(cur, out)
        if hasattr(self, "add_babble"):
            cur = self.add_babble._apply(cur, lens, out)
        if hasattr(self, "add_noise"):
            cur = self.add_noise._apply(cur, out)
        return _finish(cur, x, out, was_numpy)


class TimeDomainSpecAugment:
    """Speed perturbation, then drop_freq and drop_chunk with the library's defaults (see the module docstring)."""

    def __init__(self, speeds=[95, 100, 105], sample_rate=16000, perturb_prob=1.0, drop_freq_prob=1.0, drop_chunk_prob=1.0,
                 drop_chunk_length_low=1000, drop_chunk_length_high=2000, drop_chunk_count_low=0, drop_chunk_count_high=5,
                 drop_freq_count_low=0, drop_freq_count_high=3, drop_chunk_noise_factor=0):
        self.speeds, self.sample_rate, self.perturb_prob = speeds, sample_rate, perturb_prob
        self.drop_chunk_count_low, self.drop_chunk_count_high = drop_chunk_count_low, drop_chunk_count_high
        self.drop_chunk_length_low, self.drop_chunk_length_high = drop_chunk_length_low, drop_chunk_length_high
        self.drop_chunk_noise_factor = drop_chunk_noise_factor
        self.drop_freq_prob, self.drop_freq_count_low, self.drop_freq_count_high = drop_freq_prob, drop_freq_count_low, drop_freq_count_high
        self.drop_chunk_prob = drop_chunk_prob

    def construct(self, waves, lens, out=None):
        x, was_numpy = _rows(waves)
        cur = x
        idx = A.speed_perturb_host(len(self.speeds))  # (speed_perturb's own default perturb_prob: the example passes three arguments)
        if idx is not None:
            cur = A.speed_perturb_device(cur, self.sample_rate, self.speeds[idx])
        dec = A.drop_freq_host()
        if dec is not None:
            cur = A.drop_freq_device(cur, dec["filter"])
        lens = lens.detach().cpu().numpy() if hasattr(lens, "detach") else lens
        dec = A.drop_chunk_host(lens, cur.shape[1], cur.shape[0])
        if dec is not None:
            cur = A.drop_chunk_device(cur, dec, out=out)
        return _finish(cur, x, out, was_numpy)
