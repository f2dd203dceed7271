"""GPU: mindaudio_amd.data.augment / ecapa.spec_augment / ecapa.generate_train_data against the reference's outputs in
tests/golden/augment_goldens.npz (gen_augment_goldens.py ran the reference's own NumPy functions on the cases of augment_cases.py).

Accuracy: what can be derived is exact (samples outside dropped chunks, zeros, speed 100, decisions).  For the arithmetic the yardstick
is the fixture's `e32` - the error of a single-precision CPU evaluation of the reference's formula against its float64 output: the
device result must be within 8 x e32 in relative rms and 16 x e32 in max-abs over peak, each with a floor of 8 * 2^-24.

Measured on an MI355X (relative rms / max-abs over peak, worst over NumPy and tensor input): see the table in DESIGN.md,
"ECAPA training-data generation"."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import augment_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(HERE, "golden", "augment_goldens.npz"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return C.make_files(str(tmp_path_factory.mktemp("augment_files")))


def _seed(s):
    np.random.seed(s)
    random.seed(s)


def _errors(y, ref):
    err = np.asarray(y, np.float64) - ref
    return float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2))), float(np.abs(err).max() / np.abs(ref).max())


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_against_the_reference(torch, fix, files, name, as_tensor):
    from mindaudio_amd.data import augment as A

    case = C.CASES[name]
    conv = (lambda a: torch.from_numpy(a).cuda()) if as_tensor else (lambda a: a)
    _seed(case["seed"])
    y = case["ours"](A, files, conv)
    if as_tensor:
        assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32
        y = y.cpu().numpy()
    assert isinstance(y, np.ndarray) and y.dtype == np.float32
    y = C.flat(y, C.TIME_AXIS.get(name, -1))
    if case.get("cols") is not None:
        assert y.shape[1] == 48000
        y = y[:, case["cols"]()]
    ref = fix[name + "/out"]
    assert y.shape == ref.shape
    if case.get("exact"):
        assert ref.dtype == np.float32 and np.array_equal(y, ref)
        return
    e32 = fix[name + "/e32"]
    rms, mx = _errors(y, ref)
    print("ERRTABLE %s %s e32 %.3g %.3g gpu %.3g %.3g" % (name, "tensor" if as_tensor else "numpy", e32[0], e32[1], rms, mx))
    assert rms <= max(8 * e32[0], FLOOR), (rms, e32[0])
    assert mx <= max(16 * e32[1], FLOOR), (mx, e32[1])


def test_drop_chunk_noise_leaves_everything_else_bit_identical(torch, files):
    from mindaudio_amd.data import augment as A

    case = C.CASES["drop_chunk_noise"]
    _seed(case["seed"])
    dec = case["host"](A, files)
    _seed(case["seed"])
    x = C.X_DC()
    y = case["ours"](A, files, lambda a: a)
    keep = np.ones(x.shape, bool)
    for i in range(x.shape[0]):
        for lo, hi in dec["intervals"][i]:
            keep[i, lo:hi] = False
    assert keep.sum() < keep.size and np.array_equal(y[keep], x[keep])
    amp = np.abs(C.f64(x)).sum(axis=1) / (C.L_DC() * x.shape[1])
    assert np.all(np.abs(y[~keep]) <= (2 * amp * 0.5)[np.nonzero(~keep)[0]] * (1 + 1e-6))


def test_strided_rows_give_the_contiguous_result(torch):
    """Every entry point takes row strides: rows that are a slice of a wider matrix, and outputs written into such a slice (with the
    zero padding behind a shorter result), equal the contiguous call bit for bit."""
    from mindaudio_amd import _lib, ops
    from mindaudio_amd.data import augment as A

    x = torch.from_numpy(C.rows((1000, 21000, 41000, 61000, 71000), 3001)).cuda()
    wide = torch.full((5, 4000), 7.0, device="cuda")
    wide[:, 500:3501] = x
    xs = wide[:, 500:3501]
    assert not xs.is_contiguous()
    stats = ops.aug_row_stats(x)
    assert torch.equal(ops.aug_row_stats(xs), stats)
    ref64 = np.abs(C.f64(x.cpu().numpy())).sum(axis=1)
    assert np.abs(stats[:, 0].cpu().numpy() - ref64).max() <= 1e-9 * ref64.max()
    assert torch.equal(stats[:, 2].float(), x.abs().amax(dim=1))

    def into_slice(fn, n_out=3301):
        out = torch.full((5, 5000), 3.0, device="cuda")
        view = out[:, 1000:1000 + n_out]
        assert fn(xs, view) is view
        assert bool((out[:, :1000] == 3.0).all()) and bool((out[:, 1000 + n_out:] == 3.0).all())
        assert bool((view[:, 3001:] == 0.0).all())
        return view[:, :3001]

    h = torch.from_numpy(A.compose_drop_filter([0.3]).astype(np.float32)).cuda()
    assert torch.equal(into_slice(lambda a, o: ops.aug_circular_fir(a, h, out=o)), ops.aug_circular_fir(x, h))
    taps = torch.from_numpy(C.K_RV()).cuda()
    assert torch.equal(into_slice(lambda a, o: ops.aug_fft_conv(a, taps, 30, stats, out=o)), ops.aug_fft_conv(x, taps, 30, stats))
    noise = torch.from_numpy(C.rows((5000,), 3001)[0]).cuda()
    assert torch.equal(into_slice(lambda a, o: ops.aug_mix(a, _lib.AUG_MIX_NOISE, stats, noise=noise, gain=0.3, out=o)),
                       ops.aug_mix(x, _lib.AUG_MIX_NOISE, stats, noise=noise, gain=0.3))
    iv = torch.tensor([[[10, 500], [400, 700]], [[0, 0], [2990, 3001]], [[5, 6], [0, 0]], [[0, 3001], [1, 2]], [[0, 0], [0, 0]]])
    assert torch.equal(into_slice(lambda a, o: ops.aug_drop_chunks(a, iv, out=o)), ops.aug_drop_chunks(x, iv))
    assert torch.equal(ops.aug_babble_sum(xs, 3), ops.aug_babble_sum(x, 3))
    assert torch.equal(ops.aug_babble_sum(x, 2)[0], x[4] + x[3])
    # a cut: fewer output columns than samples
    cut = torch.empty((5, 2000), device="cuda")
    ops.aug_drop_chunks(x, iv, out=cut)
    assert torch.equal(cut, ops.aug_drop_chunks(x, iv)[:, :2000])


def test_amplitude_helpers(torch):
    from mindaudio_amd.data import augment as A
    from mindaudio_amd.data import processing, spectrum

    x = C.rows((3000, 43000), 2000)
    x64 = C.f64(x)
    amp = np.abs(x64).sum(axis=1, keepdims=True)
    got = spectrum.compute_amplitude(x, 1500.0)
    assert got.shape == (2, 1) and got.dtype == np.float32 and np.abs(got - amp / 1500).max() <= 2e-7 * (amp / 1500).max()
    assert np.abs(spectrum.compute_amplitude(x, amp_type="peak") - np.abs(x64).max(axis=1, keepdims=True)).max() == 0
    with pytest.raises(TypeError):
        spectrum.compute_amplitude(x, amp_type="rms")
    assert spectrum.dB_to_amplitude(np.array([10.0]), 1, 1)[0] == pytest.approx(10.0, rel=1e-15)
    want = x64 / (amp / 2000 + 1e-14) * 0.25
    got = processing.rescale(x, 0.25, lengths=2000)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 4e-7 * np.abs(want).max()
    got = processing.unitarize(torch.from_numpy(x).cuda(), amp_type="peak")
    assert np.abs(got.cpu().numpy() - x64 / (np.abs(x64).max(axis=1, keepdims=True) + 1e-14)).max() <= 4e-7
    with pytest.raises(AssertionError):
        processing.rescale(x, 1.0, amp_type="max")
    got = A.rms_normalize(x)
    want = x64 / (np.sqrt(np.square(x64).mean()) + 1e-8)
    assert np.abs(got - want).max() <= 4e-7 * np.abs(want).max()
    assert np.abs(A.caculate_rms(x) - np.sqrt(np.square(x64).mean(axis=-1))).max() <= 2e-7 * np.sqrt(np.square(x64).mean())


def _augmenters(files):
    from mindaudio_amd.ecapa.spec_augment import EnvCorrupt, TimeDomainSpecAugment

    env = dict(reverb_csv=files["reverb_csv"], noise_csv=files["noise_csv"], noise_snr_low=0, noise_snr_high=15)
    return [TimeDomainSpecAugment(sample_rate=16000, speeds=[100]), TimeDomainSpecAugment(sample_rate=16000, speeds=[95, 100, 105]),
            EnvCorrupt(reverb_prob=1.0, noise_prob=0.0, **env), EnvCorrupt(reverb_prob=0.0, noise_prob=1.0, **env),
            EnvCorrupt(reverb_prob=1.0, noise_prob=1.0, **env)]


def _batch():
    return C.rows(tuple(range(500, 47000, 6000)), 48000)  # (8, 48000)


def test_augment_batch_equals_the_chain_of_single_functions(torch, files):
    from mindaudio_amd import ops
    from mindaudio_amd.data import augment as A
    from mindaudio_amd.data.features import fbank
    from mindaudio_amd.ecapa.generate_train_data import augment_batch

    x = torch.from_numpy(_batch()).cuda()
    b, n = x.shape
    _seed(31)
    feats = augment_batch(x, _augmenters(files))
    assert tuple(feats.shape) == (48, 301, 80) and feats.dtype == torch.float32 and feats.is_cuda

    def fit(w):
        out = torch.zeros((b, n), device="cuda")
        m = min(n, w.shape[1])
        out[:, :m] = w[:, :m]
        return out

    lens = np.ones(b)
    _seed(31)
    parts = [x]
    for speeds in ([100], [95, 100, 105]):
        parts.append(fit(A.drop_chunk(A.drop_freq(A.speed_perturb(x, 16000, speeds)), lens)))
    parts.append(fit(A.add_reverb(x, files["rir"], 1.0)))
    parts.append(fit(A.add_noise(x, files["noise"], 0, 15, 1.0)))
    parts.append(fit(A.add_noise(A.add_reverb(x, files["rir"], 1.0), files["noise"], 0, 15, 1.0)))
    mat = torch.cat(parts, dim=0)
    want = ops.sentence_mean_norm(fbank(mat, deltas=False, n_mels=80, left_frames=0, right_frames=0, n_fft=400,
                                        hop_length=160).transpose(1, 2).contiguous())
    # same kernels on the same rows, only the slice writes differ
    diff = (feats - want).abs().max().item()
    print("augment_batch vs assembled chain: max abs difference %.3g dB" % diff)
    assert diff <= 1e-4
    assert not torch.equal(feats[:8], feats[8:16]) and not torch.equal(feats[:8], feats[40:])


def test_chain_is_bit_reproducible(torch, files):
    from mindaudio_amd.ecapa.generate_train_data import augment_batch

    x = torch.from_numpy(_batch()).cuda()
    augs = _augmenters(files)
    _seed(32)
    first = augment_batch(x, augs).clone()
    _seed(32)
    assert torch.equal(augment_batch(x, augs), first)
    _seed(33)
    assert not torch.equal(augment_batch(x, augs), first)


def test_construct_without_out_and_no_concat(torch, files):
    from mindaudio_amd.ecapa.generate_train_data import augment_batch
    from mindaudio_amd.ecapa.spec_augment import InputNormalization

    augs = _augmenters(files)
    x = _batch()[:2, :16000]
    _seed(34)
    y = augs[1].construct(x, np.ones(2))
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape[0] == 2 and y.shape[1] in (15200, 16000, 16800)
    _seed(34)
    feats = augment_batch(x, augs, concat_augment=False)
    assert tuple(feats.shape) == (2, 101, 80)
    norm = InputNormalization(norm_type="sentence", std_norm=False).construct(feats)
    assert float(norm.mean(dim=1).abs().max()) < 1e-3


def test_generate_train_data_end_to_end(torch, files, tmp_path):
    import yaml

    from mindaudio_amd.ecapa import generate_train_data as G
    from mindaudio_amd.ecapa.speaker_verification_cosine import DatasetGenerator

    folder = os.path.dirname(files["noise_csv"])  # holds noise.csv / reverb.csv: what the example expects of data_folder
    csv_path = tmp_path / "train.csv"
    with open(csv_path, "w") as fh:
        fh.write("ID,duration,wav,start,stop,spk_id\n")
        for k, spk in enumerate(("id2", "id1", "id2", "id3")):
            fh.write("utt%d,5.999,%s,%d,%d,%s\n" % (k, C.WAV, 1000 * k, 1000 * k + 48000, spk))
    cfg = dict(train_annotation=str(csv_path), feat_folder=str(tmp_path / "feat"), data_folder=folder, sample_rate=16000,
               sentence_len=3.0, random_chunk=True, number_of_epochs=1, concat_augment=True, dataloader_options=dict(batch_size=4))
    cfg_path = tmp_path / "ecapatdnn.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    _seed(35)
    labels, feas = G.main(["--config_path", str(cfg_path)])
    assert len(labels) == len(feas) == 1
    data = DatasetGenerator(str(tmp_path / "feat"), drop=False)
    assert len(data) == 1
    fea = np.load(data.data[0])
    ids = np.load(data.label[0])
    assert fea.shape == (24, 301, 80) and fea.dtype == np.float32 and np.isfinite(fea).all()
    assert ids.shape == (24, 1) and ids[:, 0].tolist() == [0, 1, 0, 2] * 6
    assert np.abs(fea.mean(axis=1)).max() < 1e-3  # sentence mean normalisation
    assert not np.array_equal(fea[:4], fea[4:8])
