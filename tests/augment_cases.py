"""The cases of tests/golden/augment_goldens.npz, shared by the generator (which runs the reference's functions on them) and by
test_augment_cpu.py / test_augment_gpu.py (which run ours).  Inputs are cut from tests/golden/BAC009S0002W0122.wav, so the fixture
stores outputs and decisions only; the noise and impulse-response "files" are small 16-bit WAVs written by make_files().

A case is a dict:
  ref(R, f)     the reference call(s): R = the reference's augment module, f = make_files(); float64 result
  ours(A, f, c) the same through mindaudio_amd: A = data.augment, c converts a float32 input array to what is fed in (NumPy as is,
                or a device tensor)
  host(A, f)    the host halves only, in call order (no device): what test_augment_cpu.py replays
  seed          np.random.seed(seed); random.seed(seed) before each of them
  cols          optional: the output columns (time axis, the last one after `flat`) kept in the fixture
  exact         the result is derivable bit for bit (stored as float32)
"""
import os
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WAV = os.path.join(HERE, "golden", "BAC009S0002W0122.wav")
_cache = {}


def wav():
    if "wav" not in _cache:
        from mindaudio_amd.data.io import read

        w, sr = read(WAV)
        assert sr == 16000 and w.shape == (95984,)
        _cache["wav"] = np.asarray(w, np.float64)
    return _cache["wav"]


def rows(offsets, n):
    """(len(offsets), n) float32: segments of the wav."""
    return np.stack([wav()[o:o + n] for o in offsets]).astype(np.float32)


def _write_wav(path, samples):
    pcm = np.clip(np.round(np.asarray(samples, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes(pcm.tobytes())


def rir(offset, taps, peak, decay, gain=4.0):
    """A decaying cut of the wav with a dominant sample at index `peak` (float32)."""
    i = np.arange(taps)
    r = wav()[offset:offset + taps] * np.exp(-np.abs(i - peak) / decay) * gain
    r[peak] = 0.9
    return r.astype(np.float32)


def make_files(folder):
    """Writes the noise / impulse-response WAVs and their csv files into `folder`; returns the path lists."""
    os.makedirs(folder, exist_ok=True)
    noise, rirs = [], []
    for k, (off, n) in enumerate(((10000, 700), (30000, 1100), (52000, 900))):
        path = os.path.join(folder, "noise_%d.wav" % k)
        _write_wav(path, wav()[off:off + n] * 0.5)
        noise.append(path)
    for k, (off, taps, peak, decay) in enumerate(((20000, 400, 30, 50.0), (61000, 250, 7, 30.0))):
        path = os.path.join(folder, "rir_%d.wav" % k)
        _write_wav(path, rir(off, taps, peak, decay))
        rirs.append(path)
    for name, paths in (("noise.csv", noise), ("reverb.csv", rirs)):
        with open(os.path.join(folder, name), "w") as fh:
            fh.write("ID,duration,wav,wav_format,wav_opts\n\n")
            for p in paths:
                fh.write(",".join((os.path.basename(p)[:-4], "0.05", p, "wav", "\n")))
    return {"noise": noise, "rir": rirs, "noise_csv": os.path.join(folder, "noise.csv"), "reverb_csv": os.path.join(folder, "reverb.csv")}


def sample_cols(n, extra=()):
    """Columns kept from a long output: both ends, the neighbourhood of every index in `extra` (seams), a sparse interior sample."""
    idx = set(range(0, 64)) | set(range(n - 64, n)) | set(range(97, n, 41))
    for e in extra:
        idx |= set(range(e - 24, e + 24))
    return np.array(sorted(i for i in idx if 0 <= i < n), np.int64)


def f64(x):
    return np.asarray(x, np.float64)


def flat(y, time_axis=-1):
    """(rows, time) view of an output whose time axis is `time_axis`."""
    y = np.asarray(y)
    if y.ndim == 1:
        return y[None, :]
    return np.moveaxis(y, time_axis, -1).reshape(-1, y.shape[time_axis])


TIME_AXIS = {"drop_freq_2": 1, "conv_odd": 1, "reverb_bt1": 1, "reverb_big": 1}  # [batch, time, channels] outputs; else the last


X_DF1 = lambda: rows((1000, 40000), 1500)  # noqa: E731
X_DF2 = lambda: np.stack([rows((5000, 22000), 1201), rows((47000, 70000), 1201)], axis=-1)  # noqa: E731  (2, 1201, 2)
X_CV1 = lambda: rows((3000, 33000), 1400)  # noqa: E731
K_CV1 = lambda: rir(25000, 300, 37, 60.0)  # noqa: E731
X_CV2 = lambda: rows((8000,), 500)[0]  # noqa: E731
K_CV2 = lambda: rir(26000, 800, 5, 200.0)  # noqa: E731
X_CV3 = lambda: np.stack([rows((9000,), 1001), rows((19000,), 1001)], axis=-1)  # noqa: E731  (1, 1001, 2)
K_CV3 = lambda: rir(27000, 64, 0, 20.0)  # noqa: E731
X_RV1 = lambda: rows((12000,), 2000)[0]  # noqa: E731
K_RV = lambda: rir(20000, 400, 30, 50.0)  # noqa: E731
X_RV2 = lambda: rows((14000, 44000), 1500)[:, :, None]  # noqa: E731
X_BIG = lambda: rows((2000, 46000), 48000)[:, :, None]  # noqa: E731
K_BIG = lambda: rir(40000, 16000, 300, 2000.0)  # noqa: E731
BIG_COLS = lambda: sample_cols(48000, (300, 15700, 16000, 47700))  # noqa: E731
X_AR1 = lambda: rows((16000, 56000), 1600)  # noqa: E731
X_AR2 = lambda: rows((1000, 21000, 41000, 61000), 1000).reshape(2, 2, 1000)  # noqa: E731
X_AN1 = lambda: rows((17000, 57000), 600)  # noqa: E731
X_AN2 = lambda: rows((18000, 58000), 2500)  # noqa: E731
X_BB = lambda: rows((2000, 24000, 48000, 72000), 1200)  # noqa: E731
L_BB = lambda: np.array([1.0, 0.75, 0.5, 0.9])  # noqa: E731
X_DC = lambda: rows((6000, 36000, 66000), 2400)  # noqa: E731
L_DC = lambda: np.array([1.0, 0.9, 0.95])  # noqa: E731
X_DC0 = lambda: rows((7000, 27000, 47000, 67000), 1500)  # noqa: E731
X_SP = lambda: rows((11000, 51000), 1600)  # noqa: E731
X_T = lambda: rows((13000, 53000), 3200)  # noqa: E731
X_E = lambda: rows((15000, 55000), 2000)  # noqa: E731


def _tdsa_ref(R):
    w = R.speed_perturb(f64(X_T()), 16000, [95, 100, 105])
    w = R.drop_freq(w)
    return R.drop_chunk(w, np.ones(2))


def _tdsa_host(A):
    idx = A.speed_perturb_host(3)
    from mindaudio_amd.data.processing import resampled_length

    m = resampled_length(3200, 16000, 16000 * [95, 100, 105][idx] // 100)
    return [idx, A.drop_freq_host(), A.drop_chunk_host(np.ones(2), m, 2)]


def _tdsa_ours(c):
    from mindaudio_amd.ecapa.spec_augment import TimeDomainSpecAugment

    return TimeDomainSpecAugment(sample_rate=16000, speeds=[95, 100, 105]).construct(c(X_T()), np.ones(2))


def _env_ref(R, f):
    return R.add_noise(R.add_reverb(f64(X_E()), f["rir"], 1.0), f["noise"], 0, 15, 1.0)


def _env_ours(f, c):
    from mindaudio_amd.ecapa.spec_augment import EnvCorrupt

    env = EnvCorrupt(reverb_csv=f["reverb_csv"], noise_csv=f["noise_csv"], reverb_prob=1.0, noise_prob=1.0, noise_snr_low=0,
                     noise_snr_high=15)
    return env.construct(c(X_E()), np.ones(2))


DC_SE = dict(drop_start=-2000, drop_end=-200)
DC_N = dict(noise_factor=0.5, drop_count_high=4)
DC_0 = dict(drop_count_low=0, drop_count_high=2)

CASES = {
    "drop_freq_1": dict(seed=3, ref=lambda R, f: R.drop_freq(f64(X_DF1()), drop_count_low=1, drop_count_high=1),
                        ours=lambda A, f, c: A.drop_freq(c(X_DF1()), drop_count_low=1, drop_count_high=1),
                        host=lambda A, f: A.drop_freq_host(drop_count_low=1, drop_count_high=1)),
    "drop_freq_2": dict(seed=4, ref=lambda R, f: R.drop_freq(f64(X_DF2()), drop_count_low=2, drop_count_high=2),
                        ours=lambda A, f, c: A.drop_freq(c(X_DF2()), drop_count_low=2, drop_count_high=2),
                        host=lambda A, f: A.drop_freq_host(drop_count_low=2, drop_count_high=2)),
    "conv_rot": dict(seed=0, ref=lambda R, f: R.convolve1d(f64(X_CV1()), f64(K_CV1())[None, :], rotation_index=37),
                     ours=lambda A, f, c: A.convolve1d(c(X_CV1()), K_CV1()[None, :], rotation_index=37), host=None),
    "conv_long_kernel": dict(seed=0, ref=lambda R, f: R.convolve1d(f64(X_CV2()), f64(K_CV2()), rotation_index=5),
                             ours=lambda A, f, c: A.convolve1d(c(X_CV2()), K_CV2(), rotation_index=5), host=None),
    "conv_odd": dict(seed=0, ref=lambda R, f: R.convolve1d(f64(X_CV3()), f64(K_CV3())[None, :, None]),
                     ours=lambda A, f, c: A.convolve1d(c(X_CV3()), K_CV3()[None, :, None]), host=None),
    "reverb_1d": dict(seed=0, ref=lambda R, f: R.reverberate(f64(X_RV1()), f64(K_RV())),
                      ours=lambda A, f, c: A.reverberate(c(X_RV1()), K_RV()), host=None),
    "reverb_bt1": dict(seed=0, ref=lambda R, f: R.reverberate(f64(X_RV2()), f64(K_RV())),
                       ours=lambda A, f, c: A.reverberate(c(X_RV2()), K_RV()), host=None),
    "reverb_big": dict(seed=0, cols=BIG_COLS, ref=lambda R, f: R.reverberate(f64(X_BIG()), f64(K_BIG())),
                       ours=lambda A, f, c: A.reverberate(c(X_BIG()), K_BIG()), host=None),
    "add_reverb_bt": dict(seed=5, ref=lambda R, f: R.add_reverb(f64(X_AR1()), f["rir"], 1.0),
                          ours=lambda A, f, c: A.add_reverb(c(X_AR1()), f["rir"], 1.0),
                          host=lambda A, f: A.add_reverb_host(f["rir"], 1.0)),
    "add_reverb_bct": dict(seed=6, ref=lambda R, f: R.add_reverb(f64(X_AR2()), f["rir"], 1.0),
                           ours=lambda A, f, c: A.add_reverb(c(X_AR2()), f["rir"], 1.0),
                           host=lambda A, f: A.add_reverb_host(f["rir"], 1.0)),
    "add_noise_cut": dict(seed=7, ref=lambda R, f: R.add_noise(f64(X_AN1()), f["noise"], 0, 15),
                          ours=lambda A, f, c: A.add_noise(c(X_AN1()), f["noise"], 0, 15),
                          host=lambda A, f: A.add_noise_host(600, f["noise"], 0, 15)),
    "add_noise_pieces": dict(seed=8, ref=lambda R, f: R.add_noise(f64(X_AN2()), f["noise"], 5, 20),
                             ours=lambda A, f, c: A.add_noise(c(X_AN2()), f["noise"], 5, 20),
                             host=lambda A, f: A.add_noise_host(2500, f["noise"], 5, 20)),
    "add_babble": dict(seed=9, ref=lambda R, f: R.add_babble(f64(X_BB()), L_BB(), 3, 0, 10),
                       ours=lambda A, f, c: A.add_babble(c(X_BB()), L_BB(), 3, 0, 10),
                       host=lambda A, f: A.add_babble_host(L_BB(), 1200, 3, 0, 10)),
    "drop_chunk_zero": dict(seed=10, exact=True, ref=lambda R, f: R.drop_chunk(f64(X_DC()), L_DC()),
                            ours=lambda A, f, c: A.drop_chunk(c(X_DC()), L_DC()),
                            host=lambda A, f: A.drop_chunk_host(L_DC(), 2400, 3)),
    "drop_chunk_noise": dict(seed=11, ref=lambda R, f: R.drop_chunk(f64(X_DC()), L_DC(), **DC_N),
                             ours=lambda A, f, c: A.drop_chunk(c(X_DC()), L_DC(), **DC_N),
                             host=lambda A, f: A.drop_chunk_host(L_DC(), 2400, 3, **DC_N)),
    "drop_chunk_start_end": dict(seed=12, exact=True, ref=lambda R, f: R.drop_chunk(f64(X_DC()), L_DC(), **DC_SE),
                                 ours=lambda A, f, c: A.drop_chunk(c(X_DC()), L_DC(), **DC_SE),
                                 host=lambda A, f: A.drop_chunk_host(L_DC(), 2400, 3, **DC_SE)),
    "drop_chunk_count0": dict(seed=13, exact=True, ref=lambda R, f: R.drop_chunk(f64(X_DC0()), np.ones(4), **DC_0),
                              ours=lambda A, f, c: A.drop_chunk(c(X_DC0()), np.ones(4), **DC_0),
                              host=lambda A, f: A.drop_chunk_host(np.ones(4), 1500, 4, **DC_0)),
    "speed_95": dict(seed=0, ref=lambda R, f: R.speed_perturb(f64(X_SP()), 16000, [95]),
                     ours=lambda A, f, c: A.speed_perturb(c(X_SP()), 16000, [95]), host=lambda A, f: A.speed_perturb_host(1)),
    "speed_100": dict(seed=0, exact=True, ref=lambda R, f: R.speed_perturb(f64(X_SP()), 16000, [100]),
                      ours=lambda A, f, c: A.speed_perturb(c(X_SP()), 16000, [100]), host=lambda A, f: A.speed_perturb_host(1)),
    "speed_105": dict(seed=0, ref=lambda R, f: R.speed_perturb(f64(X_SP()), 16000, [105]),
                      ours=lambda A, f, c: A.speed_perturb(c(X_SP()), 16000, [105]), host=lambda A, f: A.speed_perturb_host(1)),
    "chain_time_domain": dict(seed=21, ref=lambda R, f: _tdsa_ref(R), ours=lambda A, f, c: _tdsa_ours(c),
                              host=lambda A, f: _tdsa_host(A)),
    "chain_env_corrupt": dict(seed=22, ref=lambda R, f: _env_ref(R, f), ours=lambda A, f, c: _env_ours(f, c),
                              host=lambda A, f: [A.add_reverb_host(f["rir"], 1.0), A.add_noise_host(2000, f["noise"], 0, 15, 1.0)]),
}


# ---- recording the draws ------------------------------------------------------------------------------------------------------------
def _summary(v):
    if isinstance(v, str):
        return os.path.basename(v)
    a = np.asarray(v)
    if a.size > 16:
        return {"n": int(a.size), "head": [float(t) for t in a.reshape(-1)[:4]], "sum": float(a.sum())}
    return [float(t) for t in a.reshape(-1)]


class record_draws:
    """Context manager: logs every np.random.rand / randint / uniform and random.choice call (name, arguments, result) made inside it;
    on exit `.log` also ends with the NEXT draw of both generators - the state the calls left behind."""

    def __init__(self, seed):
        self.seed, self.log = seed, []

    def __enter__(self):
        import random

        self._random = random
        self._saved = (np.random.rand, np.random.randint, np.random.uniform, random.choice)
        log = self.log

        def wrap(name, fn):
            def inner(*a, **k):
                r = fn(*a, **k)
                args = [_summary(x) if not isinstance(x, (list, tuple)) or name != "choice" else len(x) for x in a]
                args += [[key, _summary(val)] for key, val in sorted(k.items())]
                log.append([name, args, _summary(r)])
                return r
            return inner

        np.random.rand = wrap("rand", self._saved[0])
        np.random.randint = wrap("randint", self._saved[1])
        np.random.uniform = wrap("uniform", self._saved[2])
        random.choice = wrap("choice", self._saved[3])
        np.random.seed(self.seed)
        random.seed(self.seed)
        return self

    def __exit__(self, *exc):
        np.random.rand, np.random.randint, np.random.uniform, self._random.choice = self._saved
        if exc[0] is None:
            self.log.append(["next", [], [float(np.random.rand()), float(self._random.random())]])
        return False
