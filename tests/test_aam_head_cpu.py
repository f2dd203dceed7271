"""CPU: the host side of the ECAPA speaker-classification head - the cyclic learning rate, the running loss average, the sampler,
the merged-feature writer and reader, AdditiveAngularMargin's constants and the error paths that must raise before any device call."""
import math
import os
import pickle

import numpy as np
import pytest

from mindaudio_amd.ecapa import train_speaker_embeddings as T


def test_cyclic_learning_rate():
    f = T.learning_rate_clr_triangle_function
    for it, want in ((0, 1e-6), (130000, 1e-6), (65000, 1e-4), (32500, 5.05e-5), (97500, 5.05e-5)):
        assert abs(f(65000, 1e-4, 1e-6, it) - want) <= 1e-12, (it, f(65000, 1e-4, 1e-6, it))


def test_update_average_follows_the_recurrence():
    losses = [3.0, 1.0, 2.5, 0.25, 7.0]
    avg = 0
    want = 0.0
    for step, loss in enumerate(losses, 1):
        avg = T.update_average(loss, avg, step)
        want = want - want / step + loss / step
        assert avg == want
    assert abs(avg - np.mean(losses)) <= 1e-12


def test_distributed_sampler():
    perm0 = np.random.RandomState(seed=0).permutation(10).tolist()
    perm1 = np.random.RandomState(seed=1).permutation(10).tolist()
    samplers = [T.DistributedSampler(10, 4, r) for r in range(4)]
    first = [list(iter(s)) for s in samplers]
    assert all(len(ix) == 3 == len(s) for ix, s in zip(first, samplers))
    padded = perm0 + perm0[:2]
    for r in range(4):
        assert first[r] == padded[r::4]
    assert sorted(sum(first, [])) == sorted(padded)
    second = [list(iter(s)) for s in samplers]
    padded1 = perm1 + perm1[:2]
    for r in range(4):
        assert second[r] == padded1[r::4]
    assert list(iter(T.DistributedSampler(10, 1, 0, shuffle=False))) == list(range(10))
    assert list(iter(T.DistributedSampler(10, 4, 1, shuffle=False))) == [1, 5, 9]


def _write_batches(folder, n_files=11, rows=6, bad=None):
    rng = np.random.RandomState(3)
    feas, labels = [], []
    for i in range(n_files):
        fea = rng.randn(rows, 301, 80).astype(np.float32)
        label = rng.randint(0, 50, size=(rows if i != bad else rows - 1, 1))
        np.save(os.path.join(folder, "b%02d_fea.npy" % i), fea)
        np.save(os.path.join(folder, "b%02d_id.npy" % i), label)
        feas.append(fea)
        labels.append(label)
    with open(os.path.join(folder, "fea.lst"), "w") as fh:
        fh.writelines("b%02d_fea.npy\n" % i for i in range(n_files))
    with open(os.path.join(folder, "label.lst"), "w") as fh:
        fh.writelines("b%02d_id.npy\n" % i for i in range(n_files))
    return feas, labels


def test_data_trans_dp_layout_and_reader(tmp_path):
    src, dst = str(tmp_path / "feat"), str(tmp_path / "merge")
    os.makedirs(src)
    feas, labels = _write_batches(src)
    T.data_trans_dp(src, dst, samples_per_file=3, epoch_len=5, log=lambda *a: None)
    kept = [i for i in range(11) if (i + 1) % 5]
    assert kept == [0, 1, 2, 3, 5, 6, 7, 8, 10]  # entries 5 and 10 (1-based) are dropped
    assert sorted(os.listdir(dst)) == sorted(["%d.npy" % k for k in range(3)] + ["%d_label.npy" % k for k in range(3)] +
                                             ["ind_sample.p", "ind_label.p"])
    with open(os.path.join(dst, "ind_sample.p"), "rb") as fh:
        ind_sample = pickle.load(fh)
    with open(os.path.join(dst, "ind_label.p"), "rb") as fh:
        ind_label = pickle.load(fh)
    n = 6 * 301 * 80
    assert set(ind_sample) == set(ind_label) == {"b%02d_fea.npy" % i for i in kept}
    for pos, i in enumerate(kept):
        name = "b%02d_fea.npy" % i
        assert tuple(ind_sample[name]) == (pos // 3, (pos % 3) * n, n)
        assert tuple(ind_label[name]) == (pos // 3, (pos % 3) * 6, 6)
    for k in range(3):
        assert np.load(os.path.join(dst, "%d.npy" % k)).shape == (3 * n,)
        assert np.load(os.path.join(dst, "%d_label.npy" % k)).shape == (18,)
    ds = T.DatasetGeneratorBatch(dst)
    assert len(ds) == 9
    for pos, i in enumerate(kept):  # the file names sort in the order they were written
        fea, label = ds[pos]
        assert fea.shape == (6, 301, 80) and fea.dtype == np.float32 and label.shape == (6,)
        assert np.array_equal(fea, feas[i]) and np.array_equal(label, labels[i].reshape(-1))
    two = T.DatasetGeneratorBatch([dst, dst])
    assert len(two) == 18 and np.array_equal(two[9][0], feas[0])


def test_data_trans_dp_rejects_a_row_count_mismatch(tmp_path):
    src = str(tmp_path / "feat")
    os.makedirs(src)
    _write_batches(src, n_files=3, bad=1)
    with pytest.raises(ValueError):
        T.data_trans_dp(src, str(tmp_path / "merge"), samples_per_file=3, epoch_len=5, log=lambda *a: None)


def test_additive_angular_margin_attributes():
    from mindaudio_amd.loss import AdditiveAngularMargin

    aam = AdditiveAngularMargin(0.2, 30)
    assert (aam.margin, aam.scale, aam.easy_margin) == (0.2, 30, False)
    assert aam.cos_m == math.cos(0.2) and aam.sin_m == math.sin(0.2)
    assert aam.th == math.cos(math.pi - 0.2) and aam.mm == math.sin(math.pi - 0.2) * 0.2
    plain = AdditiveAngularMargin()
    assert (plain.margin, plain.scale, plain.easy_margin) == (0.0, 1.0, False)


def test_classifier_shape_and_unbuilt_blocks():
    import torch

    from mindaudio_amd.models import Classifier

    torch.manual_seed(0)
    c = Classifier(1, 0, 192, 77)
    assert tuple(c.weight.shape) == (77, 192) and c.weight.dtype == torch.float32 and c.weight.requires_grad
    bound = math.sqrt(6.0 / (77 + 192))  # Xavier uniform
    peak = float(c.weight.detach().abs().max())
    assert 0.9 * bound < peak <= bound
    assert tuple(Classifier(1).weight.shape) == (1211, 192)
    with pytest.raises(NotImplementedError):
        Classifier(192, lin_blocks=1)


def test_train_needs_the_frozen_trunk_key():
    with pytest.raises(NotImplementedError, match="backward"):
        T.train({"emb_size": 192, "class_num": 10})
    with pytest.raises(NotImplementedError, match="backward"):
        T.train({"emb_size": 192, "class_num": 10, "freeze_embedding_model": False})


def test_wrapper_rejects_bad_arguments_before_any_device_call():
    import torch

    from mindaudio_amd import ops

    emb, w = torch.zeros(4, 64), torch.zeros(10, 64)
    y = torch.tensor([0, 1, 2, 9])
    for bad in (torch.tensor([0, 1, 2, 10]), torch.tensor([0, -1, 2, 3]), np.array([0, 1, 2, 10])):
        with pytest.raises(ValueError):
            ops.aam_softmax_loss(emb, w, bad)
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(emb.double(), w, y)
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(emb, w.to(torch.bfloat16), y)
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(emb, w, y.float())
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(emb, w, y[:3])
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(torch.zeros(4, 128)[:, ::2], w, y)  # not contiguous
    with pytest.raises(ValueError):
        ops.aam_softmax_loss(emb, torch.zeros(10, 32), y)
    with pytest.raises(NotImplementedError):
        ops.aam_softmax_loss(torch.zeros(4, 48), torch.zeros(10, 48), y)
    with pytest.raises(NotImplementedError):
        ops.aam_softmax_loss(torch.zeros(4, 544), torch.zeros(10, 544), y)


def test_wrapper_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mindaudio_amd import ops
    from mindaudio_amd._lib import MindaudioAmdError
    from mindaudio_amd.loss import AdditiveAngularMargin

    with pytest.raises(MindaudioAmdError):
        ops.aam_softmax_loss(torch.zeros(4, 64), torch.zeros(10, 64), torch.tensor([0, 1, 2, 9]))
    with pytest.raises(MindaudioAmdError):
        AdditiveAngularMargin(0.2, 30)(torch.zeros(4, 10), torch.zeros(4, 10))


def test_entry_points_check_shapes_on_the_host():
    """The argument checks of the C ABI run before any launch, so they can be called without a device."""
    from mindaudio_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    assert lib.ma_aam_softmax_workspace_bytes(192, 192, 7205) > 0
    assert lib.ma_aam_softmax_workspace_bytes(192, 48, 7205) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_aam_softmax_workspace_bytes(192, 544, 7205) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_aam_softmax_workspace_bytes(0, 192, 7205) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_aam_softmax_workspace_bytes(4, 192, 1) == _lib.MA_ERR_INVALID_ARG
    # O(S B D + B tiles) with S <= 64: nothing of size B x N
    b, d, n = 192, 192, 7205
    assert lib.ma_aam_softmax_workspace_bytes(b, d, n) <= 64 * b * d * 4 + 4 * b * ((n + 31) // 32) * 4 + 4096
    p = 4096  # never dereferenced: the width check comes first
    assert lib.ma_aam_softmax_fwd_f32(p, p, p, 4, 48, 10, 0.2, 30.0, 0, 1e-4, p, p, p, p, p, p, p, p, p, 1 << 20, None) == \
        _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_aam_softmax_bwd_f32(p, p, p, 4, 48, 10, 30.0, 1e-4, p, p, p, p, p, p, 0.0, p, p, p, 1 << 20, None) == \
        _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_aam_softmax_fwd_f32(p, p, p, 4, 64, 10, 0.2, 30.0, 0, 1e-4, p, p, p, p, p, p, p, p, p, 16, None) == \
        _lib.MA_ERR_WORKSPACE
