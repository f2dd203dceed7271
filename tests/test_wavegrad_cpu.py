"""CPU: the host side of the WaveGrad vocoder - public names and bound symbols, the refusals (before any device call), the parameter
names, the checkpoint round trip, load_config, the plan (built and checked by the C side without a device), `_normalize` against the
reference's values, and known answers for the float64 restatement of wavegrad_cases.py, so that an error in it cannot be mirrored
silently.  The device side is test_wavegrad_gpu.py."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wavegrad_cases as C  # noqa: E402

SYMBOLS = ("ma_wavegrad_init_conv_f32", "ma_wavegrad_pack_bf16", "ma_wavegrad_last_conv_update_f32", "ma_wavegrad_workspace_bytes",
           "ma_wavegrad_forward", "ma_wavegrad_reverse")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavegrad_normalize.npz")


def test_public_names_and_bound_symbols():
    import mindaudio_amd.wavegrad.reverse as rv
    from mindaudio_amd import _build, _lib, models, wavegrad
    from mindaudio_amd.utils import ckpt

    assert callable(models.WaveGrad)
    assert callable(rv.reverse) and callable(wavegrad.load_config) and callable(wavegrad.mel_features)
    assert callable(wavegrad.read_wav) and callable(wavegrad._normalize) and callable(rv.main)
    assert callable(ckpt.convert_wavegrad_names) and callable(ckpt.wavegrad_to_reference_names)
    _build.build()
    lib = _lib.load()
    for sym in SYMBOLS:
        assert sym in _lib.PROTOTYPES and hasattr(lib, sym), sym
    assert _lib.ABI_VERSION == 4 and lib.ma_abi_version() == 4


def test_kernel_refusals_launch_nothing():
    """Argument checks come before any HIP call, so they can be exercised without a device: every one returns its MA_ERR code."""
    from mindaudio_amd import _lib

    lib = _lib.load()
    p = 4096  # never dereferenced: the call is refused first
    INV, UNS = _lib.MA_ERR_INVALID_ARG, _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_wavegrad_init_conv_f32(p, 1, 100, p, p, 4, 32, p, None) == INV          # even kernel
    assert lib.ma_wavegrad_init_conv_f32(p, 1, 100, p, p, 9, 32, p, None) == UNS          # more than 7 taps
    assert lib.ma_wavegrad_init_conv_f32(p, 1, 100, p, p, 5, 30, p, None) == UNS          # C0 % 4
    assert lib.ma_wavegrad_init_conv_f32(None, 1, 100, p, p, 5, 32, p, None) == INV
    assert lib.ma_wavegrad_init_conv_f32(p, 1, 100, p, p, 5, 32, p + 4, None) == INV      # misaligned
    assert lib.ma_wavegrad_init_conv_f32(p, 0, 100, p, p, 5, 32, p, None) == INV

    def pack(x=p, B=1, T=10, f=1, C=64, Cpad=64, halo=8, film=None, ldf=0, enc=None, lde=0, out=p, res=None):
        return lib.ma_wavegrad_pack_bf16(x, B, T, f, C, Cpad, halo, film, ldf, enc, lde, 1.0, 1.0, out, res, 1.0, None)

    assert pack(C=36) == UNS                      # C % 8
    assert pack(C=32, Cpad=32) == UNS             # Cpad % 64
    assert pack(C=128, Cpad=64) == INV            # Cpad < C
    assert pack(f=0) == INV and pack(halo=-1) == INV and pack(x=None) == INV
    assert pack(out=None) == INV                  # neither output
    assert pack(film=p, ldf=64) == INV            # the film matrix holds 2 C columns
    assert pack(film=p, ldf=130) == UNS           # 16-byte rows
    assert pack(enc=p, lde=32) == INV and pack(enc=p + 8) == INV

    def last(x=p, B=1, T=10, C=64, taps=3, ain=p, aout=p, pred=None):
        return lib.ma_wavegrad_last_conv_update_f32(x, B, T, C, p, p, taps, ain, None, 1.0, 1.0, 0.0, aout, pred, None)

    assert last(taps=2) == INV and last(taps=9) == UNS and last(C=66) == UNS and last(B=70000) == UNS
    assert last(aout=None) == INV and last(ain=None) == INV and last(x=None) == INV
    # a plan is checked before anything else
    plan = _lib.WaveGradPlan(0, 0, 1, 240, 20, 64, None)
    assert lib.ma_wavegrad_workspace_bytes(ctypes.byref(plan)) == INV
    assert lib.ma_wavegrad_forward(ctypes.byref(plan), p, p, p, 0, p, p, 1 << 20, None) == INV
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.ma_wavegrad_reverse(None, p, p, p, fp(), fp(), fp(), p, 1, 0, 1, p, 1 << 20, None) == INV


def test_plan_is_checked_by_the_library_without_a_device():
    """The op list of both geometries passes the C side's checks, its offsets stay inside the workspace the library reports, a halo
    smaller than a dilated tap's reach is refused, and a workspace one byte short is MA_ERR_WORKSPACE."""
    from mindaudio_amd import _lib
    from mindaudio_amd.models import WaveGrad

    lib = _lib.load()
    for hps, (B, frames) in ((C.SMALL, C.SMALL_SHAPE), (C.YAML, C.YAML_SHAPE)):
        m = WaveGrad(hps).prepare()
        assert m.halo == 8
        plan = m._plan(B, frames, torch.device("cpu"))
        n = lib.ma_wavegrad_workspace_bytes(ctypes.byref(plan.c))
        assert n == plan.ws_bytes > 0 and plan.c.enc_dim == sum(m.enc_dims)
        kinds = [o.kind for o in plan.ops]
        assert kinds[0] == _lib.WAVEGRAD_OP_INIT and kinds[-1] == _lib.WAVEGRAD_OP_LAST and kinds.count(_lib.WAVEGRAD_OP_LAST) == 1
        assert sum(o.once for o in plan.ops) == 2  # first_conv and its operand do not depend on the step
        p = 4096
        assert lib.ma_wavegrad_forward(ctypes.byref(plan.c), p, p, p, 0, p, p, n - 1, None) == _lib.MA_ERR_WORKSPACE
        conv = next(o for o in plan.ops if o.kind == _lib.WAVEGRAD_OP_CONV and o.dilation == 8)
        conv.halo = 7
        assert lib.ma_wavegrad_workspace_bytes(ctypes.byref(plan.c)) == _lib.MA_ERR_INVALID_ARG
        conv.halo = 8
        plan.ops[3].kind = 9
        assert lib.ma_wavegrad_workspace_bytes(ctypes.byref(plan.c)) == _lib.MA_ERR_INVALID_ARG


class _Untouchable:
    """Stands in for the device plumbing: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the device plumbing was touched (%s) before the refusal" % name)


def _changed(**kw):
    h = {k: (dict(v) if isinstance(v, dict) else v) for k, v in C.SMALL.items()}
    for path, v in kw.items():
        sec, _, key = path.partition("__")
        if key:
            h[sec][key] = v
        else:
            h[sec] = v
    return C.H(h)


@pytest.mark.parametrize("kwargs", [
    dict(dblock__init_conv_kernels=4), dict(dblock__kernel_size=[3, 2, 3]), dict(ublock__kernel_size=2), dict(first_conv__kernel_size=4),
    dict(film__kernel_size=[3, 5, 3]), dict(dblock__factor=[2, 3, 2]), dict(film__output_size=[64, 128]),
    dict(film__output_size=[64, 64, 128]), dict(ublock__hidden_size=[128, 64, 64]), dict(ublock__factor=[3, 2, 2]),
    dict(ublock__factor=[2, 3, 4]), dict(hop_samples=10), dict(dblock__init_conv_channels=36),
], ids=lambda k: "-".join("%s=%s" % kv for kv in k.items()))
def test_model_refusals_come_before_the_device(monkeypatch, kwargs):
    import mindaudio_amd.models.wavegrad as mod

    monkeypatch.setattr(mod, "_lib", _Untouchable())
    monkeypatch.setattr(mod, "_host", _Untouchable())
    with pytest.raises(NotImplementedError):
        mod.WaveGrad(_changed(**kwargs))


def test_input_refusals_come_before_the_device(monkeypatch):
    import mindaudio_amd.models.wavegrad as mod

    m = mod.WaveGrad(C.SMALL)
    monkeypatch.setattr(mod, "_lib", _Untouchable())
    monkeypatch.setattr(mod, "_host", _Untouchable())
    spec = torch.zeros((2, 64, 20))
    level = torch.tensor([0.5])
    with pytest.raises(ValueError):
        m(torch.zeros((2, 239)), level, spec)          # T != hop * frames
    with pytest.raises(ValueError):
        m(torch.zeros((2, 240)), level, spec)          # CPU tensors
    with pytest.raises(ValueError):
        m(torch.zeros((240,)), level, spec)            # rank
    with pytest.raises(ValueError):
        m(torch.zeros((2, 240)), level, spec[0])       # rank
    with pytest.raises(ValueError):
        m(torch.zeros((2, 240)), level, torch.zeros((2, 80, 20)))  # n_mels


def test_state_dict_names_and_shapes_match_the_reference_cells():
    from mindaudio_amd.models import WaveGrad

    for hps in (C.SMALL, C.YAML):
        m = WaveGrad(hps)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == C.param_shapes(hps)
    assert m.enc_dims == [32, 128, 128, 256, 512] and m.hop == 300 and m.halo == 8
    m2 = WaveGrad({k: v for k, v in C.SMALL.items()})  # a plain nested dict is accepted as well
    assert list(m2.state_dict()) == list(WaveGrad(C.SMALL).state_dict())
    # orthogonal rows for Conv1dOrthogonal, zero biases
    w = m2.UBlock[0].block2_b.weight.detach().reshape(128, -1).double()
    assert torch.allclose(w @ w.t(), torch.eye(128, dtype=torch.float64), atol=1e-5)
    assert not m2.first_conv.bias.any()


def test_checkpoint_names_round_trip(tmp_path):
    from mindaudio_amd.models import WaveGrad
    from mindaudio_amd.utils import ckpt

    src = WaveGrad(C.SMALL)
    src.load_state_dict(C.make_state(C.SMALL, 3))
    ref = ckpt.wavegrad_to_reference_names(src.state_dict())
    assert ref["DBlock.0.weight"].shape == (32, 1, 1, 5) and ref["DBlock.2.downscale1.weight"].shape == (128, 128, 1, 3)
    assert ref["FiLM.1.output_conv.weight"].shape == (256, 64, 1, 3) and ref["last_conv.bias"].shape == (1,)
    assert set(ckpt.convert_wavegrad_names(ref)) == set(src.state_dict())
    extra = {"cur_step": np.array(123, np.int32), "global_step": np.array([7], np.int32),
             "moment1.first_conv.weight": np.zeros((128, 64, 1, 3), np.float32),
             "moment2.UBlock.0.block1.bias": np.zeros((128,), np.float32)}
    path = str(tmp_path / "wavegrad.ckpt")
    ckpt.write_mindspore_ckpt(path, {**ref, **extra})
    raw = ckpt.read_mindspore_ckpt(path)
    assert raw["first_conv.weight"].ndim == 4 and int(np.asarray(raw["cur_step"]).reshape(-1)[0]) == 123
    dst = WaveGrad(C.SMALL)
    dst._prepared, dst._plans = object(), {"x": 1}
    missing, unexpected = ckpt.load_mindspore_checkpoint(dst, path)
    assert missing == [] and unexpected == []
    assert dst._prepared is None and dst._plans == {}  # the operand copies of an earlier prepare() are dropped
    want, got = src.state_dict(), dst.state_dict()
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    flat = {k: (v[:, :, 0, :] if v.ndim == 4 else v) for k, v in ref.items()}  # (out, in, k) is accepted as well
    conv = ckpt.convert_wavegrad_names(flat)
    assert all(np.array_equal(conv[k], want[k].numpy()) for k in want)
    # the other modules' dispatch is unchanged
    assert list(ckpt.convert_names({"encoder.embed.out.0.dense.weight": np.zeros((2, 2), np.float32)})) == ["encoder.embed.out.0.weight"]


def test_load_config_builds_the_attribute_object(tmp_path):
    from mindaudio_amd.models import WaveGrad
    from mindaudio_amd.wavegrad import Config, load_config

    path = tmp_path / "small.yaml"
    path.write_text(C.YAML_TEXT)
    hps = load_config(str(path))
    assert isinstance(hps, Config) and isinstance(hps.dblock, Config)
    assert hps.dblock.hidden_size == [64, 128] and hps.ublock.dilation[1] == [1, 2, 4, 8] and hps.first_conv.kernel_size == 3
    assert hps.noise_schedule_S == 60 and hps.hop_samples == 12
    assert {k: tuple(v.shape) for k, v in WaveGrad(hps).state_dict().items()} == C.param_shapes(C.SMALL)


def test_script_refuses_plot_before_anything_else(monkeypatch):
    import mindaudio_amd.wavegrad.reverse as rv

    monkeypatch.setattr(rv, "os", _Untouchable())
    with pytest.raises(NotImplementedError):
        rv.main(["--plot", "True", "--config", "/nonexistent.yaml"])


def test_normalize_equals_the_reference_bit_for_bit():
    from mindaudio_amd.wavegrad import _normalize

    g = np.load(GOLDEN)
    x, y = g["x"], g["y"]
    assert x.dtype == np.float32 and len(x) >= 150 and 0.0 in x and np.float32(1e-5) in x and np.float32(1e-6) in x and x.max() > 1e5
    got = _normalize(x.copy())
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), y.view(np.uint32))
    assert 0 < int((y == 0).sum()) and 0 < int((y == 1).sum()) and int(((y > 0) & (y < 1)).sum()) > 30


# ---- the restatement's known answers ------------------------------------------------------------------------------------------------------
def test_restatement_encoding_repeat_and_film_split():
    e = C.encoding(4, torch.tensor([0.5]))
    want = [math.sin(0.5), math.sin(0.005), math.cos(0.5), math.cos(0.005)]
    assert e.shape == (1, 4) and np.allclose(e[0].numpy(), want, rtol=0, atol=1e-15)
    x = torch.tensor([[[1.0, 2.0]]])
    assert C.repeat(x, 2).tolist() == [[[1.0, 1.0, 2.0, 2.0]]]
    o = torch.arange(12.0).reshape(1, 4, 3)
    shift, scale = C.film_split(o)
    assert torch.equal(shift, o[:, :2]) and torch.equal(scale, o[:, 2:])  # shift is the FIRST half
    # the product's host table is the same numbers, level after level
    from mindaudio_amd.models.wavegrad import positional_table

    tab = positional_table([0.5, 0.25], [4, 8])
    assert tab.shape == (2, 12) and tab.dtype == np.float32
    assert np.allclose(tab[0, :4], want, atol=1e-7) and np.allclose(tab[1, 4:], C.encoding(8, torch.tensor([0.25]))[0].numpy(), atol=1e-7)


def test_restatement_network_on_hand_weights():
    """All weights zero but chosen ones, so that the answer can be written down: with every UBlock convolution zero the output is
    last_conv's bias; with block1 and last_conv passing channel 0 through, it is first_conv's bias halved and halved again."""
    st = {k: torch.zeros(s) for k, s in C.param_shapes(C.SMALL).items()}
    audio, spec = C.inputs(C.SMALL, C.SMALL_SHAPE, 1)
    st["last_conv.bias"][0] = 0.25
    out = C.network(st, C.SMALL, audio, torch.tensor([0.3]), spec)
    assert out.shape == (2, 240) and torch.all(out == 0.25)
    # x0 = first_conv bias b on channel 0; each UBlock: block1 passes channel 0 (repeat / f), block2 = block3 = 0 (zero weights, zero film)
    # -> x = (block1 + 0) / sqrt2, then (x + 0) / sqrt2: x / 2 / f per block; last_conv centre tap on channel 0
    st["first_conv.bias"][0] = 8.0
    for n in range(3):
        st["UBlock.%d.block1.weight" % n][0, 0, 0] = 1.0
    st["last_conv.weight"][0, 0, 1] = 1.0
    out = C.network(st, C.SMALL, audio, torch.tensor([0.3]), spec)
    want = 8.0 / (2 * 2) / (2 * 3) / (2 * 2) + 0.25
    assert torch.allclose(out, torch.full_like(out, want), atol=1e-12)


def test_restatement_schedule_and_draw_order():
    level, c1, c2, sigma = C.schedule([0.36])
    a = 1 - 0.36
    assert c1[0] == 1 / a ** 0.5 and abs(c2[0] - (1 - a) / (1 - float(np.float32(a))) ** 0.5) < 1e-15 and sigma[0] == 0
    assert abs(c2[0] - (1 - a) / math.sqrt(1 - a)) < 1e-7 and level[0] == np.float32(np.float32(a) ** 0.5)
    # a one-step loop draws the initial audio and nothing else
    rng = np.random.RandomState(7)
    out, saved = C.reverse_loop(lambda audio, n: torch.zeros_like(audio), (1, 6), [0.36], rng)
    chk = np.random.RandomState(7)
    first = chk.normal(0, 1, [1, 6]).astype(np.float32).astype(np.float64)
    assert np.array_equal(out, c1[0] * first) and saved == {}
    assert rng.normal() == chk.normal()  # both streams stand at the same place: no noise draw
    # two steps: the initial audio, then ONE noise draw for n = 1, none for n = 0
    beta = [0.1, 0.2]
    level, c1, c2, sigma = C.schedule(beta)
    rng, chk = np.random.RandomState(9), np.random.RandomState(9)
    out, _ = C.reverse_loop(lambda audio, n: 0.5 * audio, (2, 5), beta, rng)
    a0 = chk.normal(0, 1, [2, 5]).astype(np.float32).astype(np.float64)
    z1 = chk.normal(0, 1, [2, 5]).astype(np.float32).astype(np.float64)
    a1 = c1[1] * (a0 - c2[1] * 0.5 * a0) + sigma[1] * z1
    want = c1[0] * (a1 - c2[0] * 0.5 * a1)
    assert np.allclose(out, want, rtol=1e-15, atol=0) and rng.normal() == chk.normal()
    ac = np.cumprod(1 - np.asarray(beta)).astype(np.float32).astype(np.float64)
    assert abs(sigma[1] - math.sqrt((1 - ac[0]) / (1 - ac[1]) * 0.2)) < 1e-15
    # the product's host schedule is the same arithmetic
    from mindaudio_amd.wavegrad.reverse import schedule, snapshot_steps

    for got, ref in zip(schedule(np.linspace(1e-4, 0.3, 6)), C.schedule(np.linspace(1e-4, 0.3, 6))):
        assert np.allclose(got, ref, rtol=1e-15, atol=0)
    assert snapshot_steps(1000) == list(range(955, 1001, 5)) and snapshot_steps(60) == list(range(15, 61, 5)) and snapshot_steps(6) == [5]
