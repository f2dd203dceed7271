"""CPU side of the CTC prefix beam search / attention rescoring modes: the fixture of tests/golden/gen_beam_goldens.py loads, the
host-side decoder-input builder reproduces the reference's hyps_in_pad / masks, the four entry points are declared and exported,
and predict() refuses the modes it does not build before it touches a device."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("ma_ctc_topk_f32", "ma_ctc_prefix_beam_search_f32", "ma_mha_small_fwd_grouped_bf16", "ma_hyp_score_f32")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "beam_goldens.npz"))


def test_fixture_loads(gold):
    assert int(gold["pb_n"]) >= 24 and int(gold["rs_n"]) >= 6
    beams = {gold["pb%d_logp" % i].shape[1] for i in range(int(gold["pb_n"]))}
    assert beams == {1, 4, 10, 16}
    scores = [gold["pb%d_score" % i] for i in range(int(gold["pb_n"]))]
    ns = [int(gold["pb%d_n" % i]) for i in range(int(gold["pb_n"]))]
    beam = [gold["pb%d_logp" % i].shape[1] for i in range(int(gold["pb_n"]))]
    assert any(n < b for n, b in zip(ns, beam))                                    # fewer hypotheses than the beam
    assert any(np.isneginf(s[:n]).any() for s, n in zip(scores, ns))               # -inf candidates inside the beam
    assert any((gold["pb%d_mask" % i][:-1] == 0).any() and gold["pb%d_mask" % i][-1] == 1 for i in range(int(gold["pb_n"])))
    assert {float(gold["rs%d_ctc_weight" % i]) for i in range(int(gold["rs_n"]))} == {0.0, 0.3, 0.5}


def test_decoder_input_matches_the_reference(gold):
    from mindaudio_amd.conformer.asr_model import decoder_input

    for i in range(int(gold["rs_n"])):
        p = "rs%d_" % i
        lens = gold[p + "len"]
        ys, masks = decoder_input(torch.from_numpy(gold[p + "hyp"]), torch.from_numpy(lens), int(gold[p + "sos"]), int(gold[p + "eos"]))
        l1 = int(lens.max()) + 1
        assert ys.shape == (len(lens), l1) and masks.shape == (len(lens), l1, l1)
        assert np.array_equal(ys.numpy(), gold[p + "hyps_in_pad"][:, :l1])
        assert np.array_equal(masks.numpy(), gold[p + "hyps_sub_masks"][:, :l1, :l1])
        # at the reference's fixed width the whole arrays agree
        ys31, m31 = decoder_input(torch.from_numpy(np.pad(gold[p + "hyp"], ((0, 0), (0, 40)))), torch.from_numpy(lens),
                                  int(gold[p + "sos"]), int(gold[p + "eos"]), L1=31)
        assert np.array_equal(ys31.numpy(), gold[p + "hyps_in_pad"]) and np.array_equal(m31.numpy(), gold[p + "hyps_sub_masks"])


def test_entry_points_declared_exported_and_bound():
    from mindaudio_amd import _build, _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mindaudio_amd.h")).read(), flags=re.S)
    _build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == 4


def _cfg(mode, ctc_weight):
    return {"decode_mode": mode, "model_conf": {"ctc_weight": ctc_weight}, "dict": "/nonexistent", "test_data": "/nonexistent"}


def test_predict_rejects_unbuilt_modes_without_a_device():
    from mindaudio_amd.conformer import predict as P

    with pytest.raises(NotImplementedError):
        P.predict(_cfg("attention", 0.3), log=lambda _l: None)
    with pytest.raises(NotImplementedError):
        P.predict(_cfg("attention_rescoring", 1.0), log=lambda _l: None)

    class _PureCtc:
        decoder = None

    with pytest.raises(NotImplementedError):
        P.predict(_cfg("attention_rescoring", 0.3), log=lambda _l: None, model=_PureCtc())
