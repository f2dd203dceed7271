"""CPU self-test of tests/convmodule_cases.py: the conditions every case kind rests on hold, a float32 evaluation of the conv module
in the kernels' operation order passes every comparator test_convmodule_exact_gpu.py uses, and every planted defect is rejected by
the comparator named in REJECTED_BY - while the whole-tensor criterion of test_conformer_ops_gpu.py::test_convmodule_one_launch
accepts the subtlest of them (two channels with exchanged BatchNorm pairs).
Also: the BatchNorm fold of models/conformer.py against torch.nn.BatchNorm1d in eval mode, in float64.  fold_batchnorm is held
directly and through _refresh_bn, its call site behind _bn_dirty; its other call site, prepare(), packs weights on the device and
cannot run here: there the function's two results go straight into the prepared "bn_scale" / "bn_shift", which the GPU encoder tests
read."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import convmodule_cases as CC  # noqa: E402
import gemm_cases as G  # noqa: E402
import train_kernel_cases as TK  # noqa: E402

_cases = {}


def case(form, kind, B, T, ks, C=256, eps=1e-5):
    key = (form, kind, B, T, ks, C, eps)
    if key not in _cases:
        _cases[key] = CC.Case(form, kind, B, T, ks, C, eps)
    return _cases[key]


def eps_of(form, kind):
    return CC.LN_EPS if form == "oproj" and kind != "glu" else (1e-5,)


@pytest.mark.parametrize("form", CC.FORMS)
def test_conditions_and_float32_model(form):
    """Every case of the GPU test: reference() asserts the kind's conditions (integer ranges, z in [16, 255], the LayerNorm rows,
    at most 2 % multi-valued intervals), and the float32 model in the kernels' order passes the comparator (whose tile only names
    the position of a wrong element)."""
    shapes = [s + (256,) for s in CC.SHAPES] + (list(CC.MID_EXTRA) if form == "mid" else [])
    worst_multi = 0.0
    for B, T, ks, C in shapes:
        for kind in CC.KINDS:
            for eps in eps_of(form, kind):
                c = case(form, kind, B, T, ks, C, eps)
                ref = c.reference()
                worst_multi = max(worst_multi, ref.get("multi", 0.0))
                for tile in (32, 64):
                    msg, pos = CC.compare(CC.model_window(c, None, tile), c, tile)
                    assert msg is None and pos <= 1, (form, kind, B, T, ks, C, eps, tile, msg)
    assert worst_multi <= CC.MULTI_CAP
    print("%s: largest share of multi-valued intervals %.3f %%" % (form, 100 * worst_multi))


def test_big_batch_case_conditions():
    B, T, ks = CC.BIG_SHAPE
    for form in CC.FORMS:
        c = case(form, "sat", B, T, ks)
        msg, _ = CC.compare(CC.model_window(c), c)
        assert msg is None, (form, msg)


# defect -> {form: the kinds whose comparator must reject it} at DEFECT_SHAPE (3 utterances of 65 frames, k = 7: tiles of 32 and of 64
# both leave a last tile of one frame); tile = the tiling the defect refers to
DEFECT_SHAPE = (3, 65, 7)
ALL = ("mid", "pw2", "cm", "oproj")
REJECTED_BY = {
    "taps_flipped": {f: ("sat", "route") for f in ALL},
    "taps_flipped_group": {f: ("sat", "route") for f in ALL},
    "halo_crosses_utterance": {f: ("sat", "route") for f in ALL},
    "halo_short": {f: ("sat", "route") for f in ALL},
    "nbr_last_zero": {f: ("sat", "route") for f in ALL},
    "nbr_first_zero": {f: ("sat", "route") for f in ALL},
    "last_tile_dropped": {f: ("sat", "route", "glu", "swish") for f in ALL},
    "bn_xor1": {f: ("sat", "route", "swish") for f in ALL},
    "bn_plus4": {f: ("sat", "route", "swish") for f in ALL},
    "bn_swap_pair": {f: ("sat", "route", "swish") for f in ALL},
    "glu_swapped": {f: ("sat", "route", "glu", "swish") for f in ALL},
    "masked_glu_zeroed": {f: ("sat",) for f in CC.FUSED},   # (one centre tap: a masked frame feeds only its own, masked, output)
    "out_of_utt_glu_b1": {f: ("sat",) for f in CC.FUSED},
    "b2_unmasked": {f: ("sat",) for f in ("pw2", "cm", "oproj")},
    "mask_on_xprime": {"oproj": ("sat", "glu", "swish")},
    "xprime_rot": {"oproj": ("sat", "route", "glu", "swish")},
    "ln_no_eps": {"oproj": ("swish",)},
    "ln_unmasked": {"oproj": ("sat",)},
}


def test_every_defect_is_listed():
    assert set(REJECTED_BY) == set(CC.DEFECTS)
    for d, forms in REJECTED_BY.items():
        assert set(forms) == set(CC.DEFECTS[d] or ALL), d


@pytest.mark.parametrize("defect", sorted(REJECTED_BY))
def test_planted_defect_is_rejected(defect):
    B, T, ks = DEFECT_SHAPE
    for form, kinds in REJECTED_BY[defect].items():
        for kind in kinds:
            eps = CC.LN_EPS[0] if defect == "ln_no_eps" else 1e-5
            c = case(form, kind, B, T, ks, 256, eps)
            for tile in (32, 64):
                msg, _ = CC.compare(CC.model_window(c, defect, tile), c, tile)
                assert msg is not None, "%s passes the %s comparator of %s (tile %d)" % (defect, kind, form, tile)


@pytest.mark.parametrize("defect", (None, "taps_flipped", "halo_crosses_utterance"))
def test_model_agrees_with_the_training_reference(defect):
    """model()'s GLU and depthwise sum against train_kernel_cases.convmid_fwd_ref on the forms that start at y, without a defect
    and with the two defects both state."""
    for kind, T, ks in (("sat", 65, 7), ("route", 129, 15), ("glu", 33, 3), ("swish", 5, 15)):
        c = case("mid", kind, 3, T, ks)
        _, _, glu, z = CC.model(c, defect, want="stages")
        acc, s = TK.convmid_fwd_ref(c.y, 3, T, 256, c.dw, torch.zeros(256), defect=defect)
        assert torch.equal(glu, s) and torch.equal(z, acc * c.sc.double() + c.sh.double()), (kind, defect)


def test_neighbour_frame_defects_at_both_tile_edges():
    """The neighbour tile's first / last frame read as zero: at 31 | 32 (32-frame tiles) and at 63 | 64 (both tilings) the routing
    case names the frame next to the edge."""
    c = case("pw2", "route", 3, 129, 15)
    for defect, tile, frames in (("nbr_last_zero", 32, (32, 64)), ("nbr_first_zero", 32, (31, 63)), ("nbr_last_zero", 64, (64,)),
                                 ("nbr_first_zero", 64, (63,))):
        bad = CC.model(c, defect, tile, torch.float32) != c.reference()["want"]
        rows = set(int(r) % 129 for r in bad.any(1).nonzero().flatten())
        assert set(frames) <= rows, (defect, tile, sorted(rows))


def test_old_criterion_on_its_own_inputs():
    """test_convmodule_one_launch's criterion on its own inputs (the table in convmodule_cases' docstring): it ACCEPTS two channels with
    exchanged BatchNorm pairs at every one of its shapes; reversed taps in a channel group and BatchNorm read from the neighbour
    channel everywhere exceed it.  All three are rejected by the exact comparators (test_planted_defect_is_rejected)."""
    for i, shape in enumerate(CC.OLD_SHAPES):
        c = CC.old_convmodule_case(*shape)
        got = {d: CC.old_convmodule_ratio(c, d) for d in CC.OLD_RATIOS}
        print("old criterion %s, error / tolerance: %s" % (shape, ", ".join("%s %.2f" % (d, r) for d, r in got.items())))
        assert got[None] < got["bn_swap_pair"] < 1, (shape, got)
        assert got["taps_flipped_group"] > 1 and got["bn_xor1"] > 1, (shape, got)
        for d, r in got.items():
            assert abs(r - CC.OLD_RATIOS[d][i]) <= 0.006, (shape, d, r)


# ---- the BatchNorm fold ------------------------------------------------------------------------------------------------------------
def _conv_module(d=16, kernel=7, dtype=torch.float64):
    from mindaudio_amd.models import conformer as M

    g = torch.Generator().manual_seed(5)
    cm = M._ConvModule(d, kernel).to(dtype)
    with torch.no_grad():
        cm.norm.weight.copy_(0.5 + torch.rand(d, generator=g))
        cm.norm.bias.copy_(torch.randn(d, generator=g))
        cm.norm.running_mean.copy_(torch.randn(d, generator=g))
        cm.norm.running_var.copy_(0.1 + 2 * torch.rand(d, generator=g))
        cm.depthwise_conv.bias.copy_(torch.randn(d, generator=g))
    return cm.eval()


def _bn_want(cm, z):
    """BatchNorm1d in eval mode of z + the depthwise bias, float64; z (N, C)."""
    with torch.no_grad():
        return cm.norm((z + cm.depthwise_conv.bias).T[None].double())[0].T


def test_batchnorm_fold_matches_batchnorm1d():
    from mindaudio_amd.models import conformer as M

    cm = _conv_module()
    z = torch.randn(50, 16, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    scale, shift = M.fold_batchnorm(cm)
    assert scale.dtype == torch.float64 and len(set(scale.tolist())) == 16 and len(set(shift.tolist())) == 16
    want = _bn_want(cm, z)
    worst, pos = TK.check_bound(z * scale + shift, {"want": want, "bound": 8 * 2.0 ** -53 * ((z * scale).abs() + shift.abs() + want.abs())})
    assert worst <= 1 and not pos, (worst, pos)
    swapped = z * scale.roll(1) + shift.roll(1)
    assert TK.check_bound(swapped, {"want": want, "bound": 1e-6 * (1 + want.abs())})[0] > 1


def test_batchnorm_refresh_after_training_uses_the_fold():
    """_refresh_bn (the eval path after _bn_dirty) writes the fold of the CURRENT running statistics into the prepared float32 tensors."""
    from mindaudio_amd.models import conformer as M

    enc = M.ConformerEncoder(80, 256, 4, 256, 2, cnn_module_kernel=7)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in enc.encoders:
            bn = l.conv_module.norm
            bn.weight.copy_(0.5 + torch.rand(256, generator=g))
            bn.bias.copy_(torch.randn(256, generator=g))
            bn.running_mean.copy_(torch.randn(256, generator=g))
            bn.running_var.copy_(0.1 + 2 * torch.rand(256, generator=g))
            l.conv_module.depthwise_conv.bias.copy_(torch.randn(256, generator=g))
    prep = {"layers": [{"bn_scale": torch.zeros(256), "bn_shift": torch.zeros(256)} for _ in enc.encoders]}
    enc._bn_dirty = True
    enc._refresh_bn(prep)
    assert enc._bn_dirty is False
    z = torch.randn(50, 256, generator=g, dtype=torch.float64)
    for l, W in zip(enc.encoders, prep["layers"]):
        cm = l.conv_module.double().eval()
        want = _bn_want(cm, z)
        sc, sh = W["bn_scale"].double(), W["bn_shift"].double()
        # the fold runs in float32 (u = 2^-24): scale = gamma / sqrt(var + eps) rounds three times (the sum's error is halved by the
        # root: <= 2.5 u, 4 u granted); shift = beta + (b - mean) scale: the difference (u), the product (u + scale's 4 u), the sum (u)
        bm = (cm.depthwise_conv.bias - cm.norm.running_mean).abs().detach()
        bound = 1.01 * G.U * (4 * (z * sc).abs() + 6 * bm * sc.abs() + sh.abs()) + 1e-12
        worst, pos = TK.check_bound(z * sc + sh, {"want": want, "bound": bound})
        assert worst <= 1 and not pos, (worst, pos)
