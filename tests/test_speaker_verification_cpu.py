"""CPU: the host side of the speaker-verification scoring - equal error rates against the reference's own results
(tests/golden/verification_goldens.npz, written by tests/golden/gen_verification_goldens.py), the C-ABI declarations of the new
entry points, the ECAPA checkpoint name maps and the argument checks that need no device."""
import importlib.util
import os
import re
import tracemalloc
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

NEW_ENTRY_POINTS = ("ma_cohort_stats_workspace_bytes", "ma_cohort_stats_f32", "ma_trial_scores_f32",
                    "ma_running_mean_sub_workspace_bytes", "ma_running_mean_sub_f32", "ma_sentence_mean_norm_f32")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_verification_goldens", os.path.join(GOLDEN, "gen_verification_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "verification_goldens.npz"))


def test_goldens_record_their_versions(gold):
    sk, sp, npv = [str(v) for v in gold["versions"]]
    assert re.match(r"\d+\.\d+", sk) and re.match(r"\d+\.\d+", sp) and re.match(r"\d+\.\d+", npv)


@pytest.mark.parametrize("name,seed", GEN.EER_CASES)
def test_get_eer_from_scores_matches_reference(gold, name, seed):
    from mindaudio_amd.metric import get_eer_from_scores

    scores, labels = GEN.make_eer_case(name, seed)
    raises = str(gold["eer_%s_raises" % name])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if raises:
            with pytest.raises(Exception) as info:
                get_eer_from_scores(scores, labels)
            assert type(info.value).__name__ == raises
            return
        eer, thr = get_eer_from_scores(scores, labels)
    want_eer, want_thr = gold["eer_%s" % name]
    print(name, "eer", eer, want_eer, "thr", thr, want_thr)
    assert abs(eer - want_eer) <= 1e-9
    if np.isinf(want_thr):
        assert thr == want_thr
    else:
        assert abs(thr - want_thr) <= 1e-9 * max(1.0, abs(want_thr))


def test_reference_quirks_are_kept(gold):
    """The docstring of metric/eer.py lists them; the goldens are what the reference returned here."""
    assert tuple(gold["eer_separable"]) == (0.5, np.inf)
    assert tuple(gold["eer_all_equal"]) == (0.5, np.inf)
    assert gold["eer_one_positive"][0] > 0.5
    assert str(gold["eer_no_negative_raises"]) == "ValueError"


def test_compute_fa_miss_shapes_and_lists():
    from mindaudio_amd.metric import compute_fa_miss, get_eer

    scores, labels = GEN.make_eer_case("overlap", 11)
    fa, miss, thr = compute_fa_miss(list(scores), list(labels))
    assert fa.shape == miss.shape == thr.shape and thr[-1] == np.inf and fa[-1] == 0.0 and miss[-1] == 1.0
    assert len(compute_fa_miss(scores, labels, return_thresholds=False)) == 2
    assert isinstance(get_eer(fa, miss), float)


@pytest.mark.parametrize("name,seed", [c for c in GEN.EER_CASES if c[0] != "no_negative"])
def test_EER_matches_reference(gold, name, seed):
    from mindaudio_amd.metric import EER

    scores, labels = GEN.make_eer_case(name, seed)
    got = EER(scores[labels == 1], scores[labels == 0])
    print(name, got, float(gold["EER_%s" % name]))
    assert abs(got - float(gold["EER_%s" % name])) <= 1e-12


def test_EER_is_not_quadratic():
    """100 000 trials: the reference's thresholds x trials matrix would be 200 000 x 100 000 booleans; peak memory stays within
    64 x the input."""
    from mindaudio_amd.metric import EER

    rng = np.random.RandomState(5)
    pos = rng.randn(30000) + 2.0
    neg = rng.randn(70000)
    tracemalloc.start()
    got = EER(pos, neg)
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    print("peak bytes", peak, "input bytes", pos.nbytes + neg.nbytes)
    assert peak <= 64 * (pos.nbytes + neg.nbytes)
    # direct count at the returned operating point's neighbourhood: EER of two unit Gaussians 2 apart is ~ Phi(-1)
    assert abs(got - 0.1587) < 0.005


def test_new_entry_points_declared_exported_bound():
    from mindaudio_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mindaudio_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % sym, header), "header lacks %s" % sym
        assert hasattr(lib, sym), "library does not export %s" % sym
        assert sym in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 4 and lib.ma_abi_version() == 4
    assert lib.ma_cohort_stats_workspace_bytes(4700, 400000) >= 256 * 400000 * 4
    assert lib.ma_cohort_stats_workspace_bytes(0, 10) < 0
    assert lib.ma_running_mean_sub_workspace_bytes(1000, 192) > 0 and lib.ma_running_mean_sub_workspace_bytes(1000, 100) < 0


def _reference_names():
    names = {}
    with open(os.path.join(GOLDEN, "ecapa_param_names.txt")) as f:
        for line in f:
            n, shape = line.split()
            names[n] = tuple(int(v) for v in shape.split(","))
    return names


def test_ecapa_checkpoint_round_trip(tmp_path):
    import torch

    from mindaudio_amd.models import EcapaTDNN
    from mindaudio_amd.utils import ckpt

    torch.manual_seed(3)
    src = EcapaTDNN(80)
    for m in src.modules():  # non-trivial BatchNorm state
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.normal_()
            m.bias.data.normal_()
    ref = ckpt.ecapa_to_reference_names(src.state_dict())
    want = _reference_names()
    assert sorted(ref) == sorted(want)
    for n, shape in want.items():
        assert tuple(ref[n].shape) == shape, n
    path = str(tmp_path / "ecapa.ckpt")
    ckpt.write_mindspore_ckpt(path, {"network." + k: v for k, v in ref.items()})
    dst = EcapaTDNN(80)
    missing, unexpected = ckpt.load_mindspore_checkpoint(dst, path)
    assert missing == [] and unexpected == []
    a, b = src.state_dict(), dst.state_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(a[k], b[k]), k


def test_ecapa_checkpoint_reports_foreign_parameters(tmp_path):
    import torch

    from mindaudio_amd.models import EcapaTDNN
    from mindaudio_amd.utils import ckpt

    src = EcapaTDNN(80, channels=(512, 512, 512, 512, 1536))
    ref = ckpt.ecapa_to_reference_names(src.state_dict())
    ref["weight"] = np.zeros((7205, 192), np.float32)  # the training Classifier's parameter
    ref["moments.fc.weight"] = np.zeros((192, 3072, 1, 1), np.float32)  # optimizer state: dropped
    path = str(tmp_path / "ecapa.ckpt")
    ckpt.write_mindspore_ckpt(path, ref)
    with pytest.raises(KeyError):
        ckpt.load_mindspore_checkpoint(EcapaTDNN(80), path)
    missing, unexpected = ckpt.load_mindspore_checkpoint(EcapaTDNN(80), path, strict=False)
    assert missing == [] and unexpected == ["weight"]


def test_conformer_name_map_is_untouched():
    from mindaudio_amd.utils import ckpt

    got = ckpt.convert_names({"network.encoder.encoders.0.conv_module.norm.gamma": np.ones(4, np.float32),
                              "encoder.encoders.0.conv_module.pointwise_conv1.conv1d.weight": np.ones((8, 4, 1, 1), np.float32)})
    assert sorted(got) == ["encoder.encoders.0.conv_module.norm.weight", "encoder.encoders.0.conv_module.pointwise_conv1.weight"]
    assert got["encoder.encoders.0.conv_module.pointwise_conv1.weight"].shape == (8, 4, 1)


def test_trial_file_parsing(tmp_path):
    from mindaudio_amd.ecapa import speaker_verification_cosine as sv

    p = tmp_path / "veri.txt"
    p.write_text("1 id1/a/0001.wav id1/b/0002.wav\n0 id1/a/0001.wav id2/c/0003.wav\n1 id2/c/0003.wav id2/c/0003.wav \n")
    index = {"id1/a/0001": 0, "id1/b/0002": 1, "id2/c/0003": 2}
    labels, enrol, test = sv.parse_trials(str(p), index, index)
    assert labels.tolist() == [1, 0, 1] and enrol.tolist() == [0, 0, 2] and test.tolist() == [1, 2, 2]
    with pytest.raises(KeyError):
        sv.parse_trials(str(p), {"id1/a/0001": 0}, index)


def test_scoring_arguments_are_checked_without_a_device(tmp_path):
    import torch

    from mindaudio_amd import ops
    from mindaudio_amd.ecapa import speaker_verification_cosine as sv

    p = tmp_path / "veri.txt"
    p.write_text("1 a.wav b.wav\n")
    table = sv.EmbeddingTable(["a", "b"], torch.zeros(2, 192))
    cohort = torch.zeros(10, 192)
    with pytest.raises(ValueError):
        sv.evaluate2(table, table, cohort, {"score_norm": "x-norm", "cohort_size": 5}, str(p), log=lambda *a: None)
    with pytest.raises(ValueError):
        sv.evaluate2(table, table, cohort, {"score_norm": "s-norm", "cohort_size": 11}, str(p), log=lambda *a: None)
    with pytest.raises(ValueError):
        sv.eval_impl({"score_norm": "snorm"}, log=lambda *a: None)
    with pytest.raises(ValueError):
        ops.cohort_stats(torch.zeros(2, 192), cohort, 11)
    with pytest.raises(ValueError):
        ops.cohort_stats(torch.zeros(2, 100), torch.zeros(10, 100), 5)  # width not a multiple of 32
    with pytest.raises(ValueError):
        ops.cohort_stats(torch.zeros(2, 544), torch.zeros(10, 544), 5)  # width above 512
    with pytest.raises(ValueError):
        ops.trial_scores(torch.zeros(2, 192), [0], [1], score_norm="x-norm")
    with pytest.raises(ValueError):
        ops.trial_scores(torch.zeros(2, 192), [0], [2])  # index outside the matrix
    with pytest.raises(ValueError):
        ops.running_mean_sub(torch.zeros(4, 192), None, 3)  # a count without a mean


def test_dataset_generator_drop(tmp_path):
    from mindaudio_amd.ecapa.speaker_verification_cosine import DatasetGenerator

    with open(tmp_path / "fea.lst", "w") as f, open(tmp_path / "label.lst", "w") as g:
        for i in range(3):
            np.save(tmp_path / ("%d_fea_mvn.npy" % i), np.full((1, 4, 80), i, np.float32))
            np.save(tmp_path / ("%d_label.npy" % i), np.array(["utt%d" % i]))
            f.write("%d_fea_mvn.npy\n" % i)
            g.write("%d_label.npy\n" % i)
    assert len(DatasetGenerator(str(tmp_path))) == 2 and len(DatasetGenerator(str(tmp_path), False)) == 3
    data, label = DatasetGenerator(str(tmp_path), False)[2]
    assert label == "utt2" and data.shape == (1, 4, 80) and data[0, 0, 0] == 2
