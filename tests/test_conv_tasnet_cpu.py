"""CPU: the host side of Conv-TasNet separation - public names and bound symbols, the refusals (raised before any device call), the
SI-SNR metrics against the reference's values, the paired overlap against the reference's 0 / 1 matrix product, the checkpoint name
mapping and the segmenting data pipeline.  The device side is test_conv_tasnet_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_tasnet_cases as C  # noqa: E402

SYMBOLS = ("ma_tasnet_stat_parts", "ma_tasnet_encode_f32", "ma_prelu_gln_stats", "ma_gln_dwconv_prelu", "ma_gln_apply_bf16",
           "ma_tasnet_decode_f32", "ma_si_snr_pairwise")


def test_public_names_and_bound_symbols():
    import mindaudio_amd.conv_tasnet.eval as ev
    from mindaudio_amd import _build, _lib, loss, metric, models, ops
    from mindaudio_amd.conv_tasnet import DatasetGenerator  # noqa: F401
    from mindaudio_amd.utils import ckpt

    assert callable(models.ConvTasNet) and callable(loss.Convtasnet_Loss)
    assert callable(metric.cal_SISNR) and callable(metric.cal_SISNRi) and not hasattr(metric, "cal_SDRi")
    assert callable(ops.si_snr_pit) and callable(ops.si_snr_pairwise)
    assert callable(ckpt.convert_conv_tasnet_names) and callable(ckpt.conv_tasnet_to_reference_names)
    assert callable(ev.evaluate) and callable(ev.main) and ev.BATCH == 8
    _build.build()
    lib = _lib.load()
    for sym in SYMBOLS:
        assert sym in _lib.PROTOTYPES and hasattr(lib, sym), sym
    assert _lib.ABI_VERSION == 4
    # the partial count is a host function: 8192 values a tile
    assert lib.ma_tasnet_stat_parts(3199, 512) == 200 and lib.ma_tasnet_stat_parts(37, 128) == 1
    assert lib.ma_tasnet_stat_parts(300, 128) == 5 and lib.ma_tasnet_stat_parts(300, 100) == 0


def test_kernel_refusals_launch_nothing():
    """Argument checks come before any HIP call, so they can be exercised without a device: every one returns its MA_ERR code."""
    from mindaudio_amd import _lib

    lib = _lib.load()
    p = 4096  # never dereferenced: the call is refused first
    assert lib.ma_tasnet_encode_f32(p, 1, 100, 100, p, 19, 64, p, p, None) == _lib.MA_ERR_UNSUPPORTED      # odd L
    assert lib.ma_tasnet_encode_f32(p, 1, 100, 100, p, 20, 96, p, p, None) == _lib.MA_ERR_UNSUPPORTED      # N % 64
    assert lib.ma_tasnet_encode_f32(p, 1, 10, 10, p, 20, 64, p, p, None) == _lib.MA_ERR_INVALID_ARG        # T < L
    assert lib.ma_tasnet_encode_f32(None, 1, 100, 100, p, 20, 64, p, p, None) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_prelu_gln_stats(p, 1, 10, 100, p, p, p, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_prelu_gln_stats(p, 0, 10, 128, p, p, p, None) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_gln_dwconv_prelu(p, 1, 10, 128, p, p, 5, 1, p, 2 * p, p, None) == _lib.MA_ERR_UNSUPPORTED  # P != 3
    assert lib.ma_gln_dwconv_prelu(p, 1, 10, 128, p, p, 3, 0, p, 2 * p, p, None) == _lib.MA_ERR_INVALID_ARG  # dilation < 1
    assert lib.ma_gln_dwconv_prelu(p, 1, 10, 128, p, p, 3, 1, p, p, p, None) == _lib.MA_ERR_INVALID_ARG      # in place
    assert lib.ma_gln_apply_bf16(p, 1, 10, 32, p, p, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_tasnet_decode_f32(p, p, 1, 10, 2, 64, p, 21, 0, p, None) == _lib.MA_ERR_UNSUPPORTED      # odd L
    assert lib.ma_tasnet_decode_f32(p, p, 1, 10, 2, 64, p, 66, 0, p, None) == _lib.MA_ERR_UNSUPPORTED      # L > 64
    assert lib.ma_tasnet_decode_f32(p, p, 1, 10, 2, 1024, p, 20, 0, p, None) == _lib.MA_ERR_UNSUPPORTED    # N > 768
    assert lib.ma_tasnet_decode_f32(p, p, 1, 10, 2, 64, p, 20, 2, p, None) == _lib.MA_ERR_INVALID_ARG      # unknown overlap
    assert lib.ma_si_snr_pairwise(p, p, p, 1, 9, 100, p, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_si_snr_pairwise(p, p, None, 1, 2, 100, p, None) == _lib.MA_ERR_INVALID_ARG


class _Untouchable:
    """Stands in for the device plumbing: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the device plumbing was touched (%s) before the refusal" % name)


@pytest.mark.parametrize("kwargs", [
    dict(causal=True), dict(P=2), dict(P=4), dict(P=5), dict(P=1), dict(N=96), dict(B=100), dict(H=130), dict(L=21), dict(L=15),
], ids=lambda k: "-".join("%s=%s" % kv for kv in k.items()))
def test_model_refusals_come_before_the_device(monkeypatch, kwargs):
    import mindaudio_amd.models.conv_tasnet as mod

    monkeypatch.setattr(mod, "_lib", _Untouchable())
    monkeypatch.setattr(mod, "_host", _Untouchable())
    args = dict(N=64, L=20, B=64, H=128, P=3, X=2, R=1, C=2)
    args.update(kwargs)
    with pytest.raises(NotImplementedError):
        mod.ConvTasNet(**args)


def test_model_accepts_the_ignored_arguments_and_names_its_parameters_as_the_reference():
    from mindaudio_amd.models import ConvTasNet

    cfg = dict(N=64, L=20, B=64, H=128, P=3, X=3, R=2, C=2)
    m = ConvTasNet(**cfg, norm_type="cLN", mask_nonlinear="softmax")  # both ignored, as in the reference
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == C.param_shapes(**cfg)
    assert [b.dilation for b in m.blocks()] == [1, 2, 4, 1, 2, 4]
    assert m.num_frames(3010) == 300 and m.num_frames(339) == 32
    with pytest.raises(ValueError):
        ConvTasNet(**cfg, overlap="hann")


def test_pit_refuses_more_than_four_sources_before_the_device(monkeypatch):
    from mindaudio_amd import ops

    monkeypatch.setattr(ops, "_lib", _Untouchable())
    with pytest.raises(NotImplementedError):
        ops.si_snr_pit(torch.zeros((1, 5, 10)), torch.zeros((1, 5, 10)), [10])


def test_eval_refuses_cal_sdr_before_anything_else():
    from mindaudio_amd.conv_tasnet.eval import evaluate

    with pytest.raises(NotImplementedError):
        evaluate({"cal_sdr": 1})


def test_metrics_equal_the_reference_values():
    from mindaudio_amd.metric import cal_SISNR, cal_SISNRi

    g = np.load(C.GOLDENS)
    n = len(g["sisnr"])
    assert n >= 6
    for i in range(n):
        got = cal_SISNR(g["ref%d" % i], g["est%d" % i])  # float32 in, float64 inside
        assert abs(got - g["sisnr"][i]) <= 1e-12 * max(1.0, abs(g["sisnr"][i])), (i, got, g["sisnr"][i])
    assert not g["ref3"].any() and g["sisnr"][3] == pytest.approx(-80.0, abs=1e-9)  # the silent reference
    assert np.array_equal(g["ref4"], g["est4"]) and g["sisnr"][4] > 100.0           # the estimate equal to the reference
    got = cal_SISNRi(g["src_ref"], g["src_est"], g["mix"])
    assert abs(got - float(g["sisnri"])) <= 1e-12 * max(1.0, abs(float(g["sisnri"])))


def test_paired_overlap_is_the_reference_matrix_product():
    """K = 7, L = 20: out[k L/2 + j] = frame_k[j] + frame_k[j + L/2] equals the explicit product with the 0 / 1 matrix built as
    conv_tasnet.py:113-119 builds it; the L / 2 trailing samples are the model's zero pad; the true overlap-add differs.

    This checks the YARDSTICK only: both sides are helpers of conv_tasnet_cases.py, no product code runs, and the test passes without
    the feature.  There is no CPU path for the decoder; the product's paired overlap is checked against these helpers on the device,
    in test_conv_tasnet_gpu.py::test_decode.  It is no coverage of the decoder."""
    g = torch.Generator().manual_seed(5)
    frames = torch.randn((2, 2, 7, 20), generator=g, dtype=torch.float64)
    want = C.overlap_paired_reference(frames)
    got = C.overlap_paired(frames)
    assert want.shape == (2, 2, 70) and got.shape == (2, 2, 80)
    assert torch.equal(got[..., :70], want) and not got[..., 70:].any()
    alpha = C.paired_matrix(7)
    assert alpha.shape == (14, 7) and alpha.sum() == 14 and alpha[2, 1] == 1 and alpha[3, 1] == 1 and alpha[4, 1] == 0
    true = C.overlap_true(frames)
    assert true.shape == (2, 2, 80) and not torch.allclose(true, got)
    assert torch.allclose(true[..., :10], frames[:, :, 0, :10]) and torch.allclose(true[..., 70:], frames[:, :, 6, 10:])
    assert torch.allclose(true[..., 10:20], frames[:, :, 0, 10:] + frames[:, :, 1, :10])


def test_checkpoint_names_round_trip(tmp_path):
    from mindaudio_amd.models import ConvTasNet
    from mindaudio_amd.utils import ckpt

    cfg = dict(N=64, L=20, B=64, H=128, P=3, X=2, R=2, C=2)
    src = ConvTasNet(**cfg)
    src.load_state_dict(C.make_state(cfg, 3))
    ref = ckpt.conv_tasnet_to_reference_names(src.state_dict())
    assert ref["encoder.conv1d_U.weight"].shape == (64, 1, 1, 20)
    assert ref["separator.temporal_conv_net.1.0.dsconv.depthwise_conv.weight"].shape == (128, 1, 1, 3)
    assert ref["separator.temporal_conv_net.0.1.prelu.w"].shape == (1,) and ref["decoder.basis_signals.weight"].shape == (20, 64)
    assert not [k for k in ref if k.endswith("prelu.weight")]
    assert set(ckpt.convert_conv_tasnet_names(ref)) == set(src.state_dict())
    # what a training checkpoint may carry besides: the cells' second registration and the optimizer state
    extra = {"separator.network.1.weight": ref["separator.bottleneck_conv1x1.weight"],
             "separator.temporal_conv_net.0.0.net.0.weight": ref["separator.temporal_conv_net.0.0.conv1x1.weight"],
             "moment1.encoder.conv1d_U.weight": np.zeros((64, 1, 1, 20), np.float32), "global_step": np.array([7], np.int32)}
    path = str(tmp_path / "tasnet.ckpt")
    ckpt.write_mindspore_ckpt(path, {**ref, **extra})
    raw = ckpt.read_mindspore_ckpt(path)
    assert raw["separator.mask_conv1x1.weight"].ndim == 4 and "separator.temporal_conv_net.0.0.dsconv.prelu.w" in raw
    dst = ConvTasNet(**cfg)
    dst._prepared = object()
    missing, unexpected = ckpt.load_mindspore_checkpoint(dst, path)
    assert missing == [] and unexpected == []
    assert dst._prepared is None  # the bf16 copies of an earlier prepare() are dropped
    want, got = src.state_dict(), dst.state_dict()
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    # (out, in, k) conv weights are accepted as well
    flat = {k: (v[:, :, 0, :] if v.ndim == 4 else v) for k, v in ref.items()}
    conv = ckpt.convert_conv_tasnet_names(flat)
    assert all(np.array_equal(conv[k], want[k].numpy()) for k in want)
    # the other modules' dispatch is unchanged
    assert list(ckpt.convert_names({"encoder.embed.out.0.dense.weight": np.zeros((2, 2), np.float32)})) == \
        ["encoder.embed.out.0.weight"]


def test_dataset_generator_segments_orders_and_drops(tmp_path):
    from mindaudio_amd.conv_tasnet import DatasetGenerator

    written = C.make_dataset(str(tmp_path), [4000, 3000, 9000])  # listed out of order: the generator sorts, longest first
    lines = []
    ds = DatasetGenerator(str(tmp_path), 4, sample_rate=8000, segment=0.5, log=lines.append)
    assert lines == ["Drop 1 utts(0.00 h) which is short than 4000 samples"] and ds.dropped == 1
    assert len(ds) == 4  # 9000 -> 0:4000, 4000:8000 and the last 4000; 4000 -> one; 3000 dropped
    s1, s2 = written[9000]
    for i, sl in enumerate((slice(0, 4000), slice(4000, 8000), slice(5000, 9000))):
        mix, n, src = ds[i]
        assert n == 4000 and mix.dtype == np.float32 and src.shape == (2, 4000)
        assert np.array_equal(src[0], (s1[sl] / 32768.0).astype(np.float32)) and np.array_equal(src[1], (s2[sl] / 32768.0).astype(np.float32))
    assert np.array_equal(ds[3][2][0], (written[4000][0] / 32768.0).astype(np.float32))
    # the group limit: with 3 the two utterances fall into two groups (same segments); with 2 the 9000-sample utterance, which alone
    # gives 3 segments, is skipped as the reference skips it
    assert len(DatasetGenerator(str(tmp_path), 3, segment=0.5, log=lines.append)) == 4
    only = DatasetGenerator(str(tmp_path), 2, segment=0.5, log=lines.append)
    assert len(only) == 1 and np.array_equal(only[0][2][1], (written[4000][1] / 32768.0).astype(np.float32))
