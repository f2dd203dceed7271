"""GPU: the five inference conv-module kernels - convmodule_mid_kernel (conformer_kernels.hip), convmid_pw2_kernel,
convmodule_kernel<false>, convmodule_kernel<true> and convmodule64_kernel (convmid_pw2.hip) - against the exact references of
tests/convmodule_cases.py (the case kinds, the conditions they rest on and the planted defects: its docstring;
test_convmodule_cases_cpu.py shows that the comparators used here reject each of them).  Every launch goes through the C ABI:
outputs and the in-place x sit in a guard-banded window (canary rows above and below, canary columns at ld = width + 8), the inputs
y, a, ctx and x of the out-of-place form in buffers with NaN padding columns and NaN rows before the first and after the last
utterance, the mask between two NaNs.  After every launch the canaries are intact, every input is bit-unchanged and a second
launch gives the same bits.

ma_attn_out_convmodule_bf16 runs on convmodule64_kernel in this process and on the 32-frame convmodule_kernel<true>
(MINDAUDIO_AMD_CONVMOD=t32) in one fresh child process: test_t32_kernel_in_a_child_process.

Measured on an MI355X (printed on every run, pytest -s; "exact": bit for bit, no figure; intervals: the worst position of an output
inside a multi-valued interval, 1 = at an end, and the largest share of multi-valued intervals over the shapes):
    kernel                      sat     route    glu (position, multi-valued)   swish (position, multi-valued)
    convmodule_mid_kernel       exact   exact    0, 0 %                          0, 0 %        (also C = 264 and k = 31)
    convmid_pw2_kernel          exact   exact    0, 0 %                          0, 0 %
    convmodule_kernel<false>    exact   exact    0, 0 %                          0, 0 %
    convmodule64_kernel         exact   exact    0, 0 %                          1, 0.391 %    (both eps; B = 40, T = 65: exact)
    convmodule_kernel<true>     exact   exact    0, 0 %                          1, 0.391 %    (both eps; B = 40, T = 65: exact)
No output lay outside its interval; 0 %: every interval of every shape holds a single bf16 number, so those checks are bit for bit
too.  The 0.391 % are the eps = 4096 rows of the Swish kind (z no integer), where an output sat at an end of a two-number interval.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import convmodule_cases as CC  # noqa: E402
import train_kernel_cases as TK  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
T32 = os.environ.get("MINDAUDIO_AMD_CONVMOD", "")[:3] == "t32"
KERNEL = {"mid": "convmodule_mid_kernel", "pw2": "convmid_pw2_kernel", "cm": "convmodule_kernel<false>",
          "oproj": "convmodule_kernel<true>" if T32 else "convmodule64_kernel"}
TILE = {"mid": 32, "pw2": 32, "cm": 32, "oproj": 32 if T32 else 64}


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _lib

    assert torch.cuda.is_available()
    return _lib.load()


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _stream():
    from mindaudio_amd import _host

    return _host.current_stream_ptr()


def _d(x):
    return x.to(DEV).contiguous()


def report(name, worst=None, multi=None):
    if worst is None:
        print("%-44s exact" % name)
    else:
        print("%-44s worst position inside an interval %.3g, multi-valued intervals %.3f %%" % (name, worst, 100 * multi))


class Padded:
    """A (rows, width) input inside a NaN-filled device buffer: `pre` rows before it, `post` after it, 8 NaN columns behind every row."""

    def __init__(self, x, pre=2, post=3):
        rows, width = x.shape
        self.buf = torch.full((pre + rows + post, width + 8), float("nan"), dtype=x.dtype, device=DEV)
        self.view = self.buf[pre:pre + rows, :width]
        self.view.copy_(x)
        self.ld = width + 8
        self.before = self.buf.cpu()

    def unchanged(self):
        return TK.check_exact(self.buf, {"want": self.before})[0] == 0


_packed = {}


def _pack(lib, c, name):
    key = (c.form, c.kind, name)
    if key not in _packed:
        w = _d(getattr(c, name))
        n = lib.ma_gemm_k256_packed_bytes(w.shape[0], 256)
        assert n == w.shape[0] * 256 * 2
        buf = torch.empty(n, dtype=torch.uint8, device=DEV)
        assert lib.ma_gemm_k256_pack_bf16(_ptr(w), w.stride(0), w.shape[0], 256, _ptr(buf), _stream()) == 0
        torch.cuda.synchronize()
        _packed[key] = (buf, getattr(c, name).clone())
    buf, w = _packed[key]
    assert torch.equal(w, getattr(c, name)), "the weights of a (form, kind) must not depend on the shape"
    return buf


def run_case(lib, c, dw=None, sc=None, sh=None):
    """Two launches of c.form on the inputs of c -> (message or None, worst position inside a multi-valued interval).
    dw, sc, sh: hand the kernel these instead of the case's own (test_wrong_parameters_are_noticed)."""
    form, M = c.form, c.B * c.T
    dw, sc, sh = _d(c.dw if dw is None else dw), _d(c.sc if sc is None else sc), _d(c.sh if sh is None else sh)
    inputs, mask = [], None
    if c.mask is not None and form != "mid":
        mbuf = torch.full((M + 2,), float("nan"), device=DEV)
        mbuf[1:M + 1] = c.mask
        mask = mbuf[1:M + 1]
    if form in ("mid", "pw2"):
        src = Padded(c.y)
    elif form == "cm":
        src = Padded(c.a)
    else:
        src, xin = Padded(c.ctx), Padded(c.x_in)
        inputs.append(xin)
        assert xin.ld == 264
    inputs.append(src)
    if form != "mid":
        p2, b2 = _pack(lib, c, "w2"), _d(c.b2)
    if form in CC.FUSED:
        p1, b1 = _pack(lib, c, "w1"), _d(c.b1)
    if form == "oproj":
        po, bo, lg, lb = _pack(lib, c, "wo"), _d(c.bo), _d(c.gamma), _d(c.beta)
    wins = []
    for _ in range(2):
        if form == "mid":
            win = CC.ld_window(M, c.C, BF16, DEV).snapshot()
            rc = lib.ma_convmodule_mid_bf16(_ptr(src.view), src.ld, c.B, c.T, c.C, _ptr(dw), c.ks, _ptr(sc), _ptr(sh), _ptr(win.view),
                                            win.ld, _stream())
        else:
            win = CC.ld_window(M, 256, F32, DEV)
            if form != "oproj":
                win.view.copy_(c.x0)
            win.snapshot()
            assert win.ld == 264
            if form == "pw2":
                rc = lib.ma_convmid_pw2_bf16(_ptr(src.view), src.ld, c.B, c.T, 256, _ptr(dw), c.ks, _ptr(sc), _ptr(sh), _ptr(p2), _ptr(b2),
                                             _ptr(mask), _ptr(win.view), win.ld, _stream())
            elif form == "cm":
                rc = lib.ma_convmodule_bf16(_ptr(src.view), src.ld, c.B, c.T, 256, _ptr(p1), _ptr(b1), _ptr(dw), c.ks, _ptr(sc), _ptr(sh),
                                            _ptr(p2), _ptr(b2), _ptr(mask), _ptr(win.view), win.ld, _stream())
            else:
                rc = lib.ma_attn_out_convmodule_bf16(_ptr(src.view), src.ld, _ptr(po), _ptr(bo), _ptr(lg), _ptr(lb), c.eps, c.B, c.T, 256,
                                                     _ptr(p1), _ptr(b1), _ptr(dw), c.ks, _ptr(sc), _ptr(sh), _ptr(p2), _ptr(b2), _ptr(mask),
                                                     _ptr(xin.view), _ptr(win.view), win.ld, _stream())
        assert rc == 0, (form, rc)
        torch.cuda.synchronize()
        wins.append(win)
    msg, pos = CC.compare(wins[0], c, TILE[form])
    if msg is None and not all(p.unchanged() for p in inputs):
        msg = "an input was written"
    if msg is None and mask is not None:
        if not (bool(torch.isnan(mbuf[0])) and bool(torch.isnan(mbuf[-1])) and torch.equal(mask.cpu(), c.mask)):
            msg = "the mask was written"
    if msg is None and TK.check_exact(wins[1].buf, {"want": wins[0].buf.cpu()})[0] != 0:
        msg = "the second launch gives other bits"
    return msg, pos


def run_kind(lib, form, kind, shapes):
    worst, multi = 0.0, 0.0
    for B, T, ks, C in shapes:
        for eps in (CC.LN_EPS if form == "oproj" and kind != "glu" else (1e-5,)):
            c = CC.Case(form, kind, B, T, ks, C, eps)
            msg, pos = run_case(lib, c)
            assert msg is None, "%s %s B %d T %d k %d C %d eps %g: %s" % (KERNEL[form], kind, B, T, ks, C, eps, msg)
            assert pos <= 1
            worst, multi = max(worst, pos), max(multi, c.reference().get("multi", 0.0))
    name = "%s %s" % (KERNEL[form], kind)
    if kind in ("sat", "route"):
        report(name)
    else:
        report(name, worst, multi)


SHAPES = [s + (256,) for s in CC.SHAPES]


@pytest.mark.parametrize("kind", CC.KINDS)
@pytest.mark.parametrize("form", ("mid", "pw2", "cm"))
def test_kernel(lib, form, kind):
    run_kind(lib, form, kind, SHAPES)


@pytest.mark.parametrize("kind", CC.KINDS)
def test_oproj_kernel(lib, kind):
    """ma_attn_out_convmodule_bf16 (the kernel of this process: KERNEL["oproj"]), both eps of LN_EPS where the kind allows."""
    run_kind(lib, "oproj", kind, SHAPES)


@pytest.mark.parametrize("kind", CC.KINDS)
def test_mid_second_channel_block_and_k31(lib, kind):
    """convmodule_mid_kernel alone takes C != 256 (C = 264: a second block of 8 channels) and k up to 31 (the per-tap path)."""
    run_kind(lib, "mid", kind, CC.MID_EXTRA)


@pytest.mark.parametrize("form", ("mid", "pw2", "cm"))
def test_many_utterances_of_65_frames(lib, form):
    """B = 40, T = 65: many workgroups with a single live frame."""
    run_kind(lib, form, "sat", [CC.BIG_SHAPE + (256,)])


def test_oproj_many_utterances_of_65_frames(lib):
    """... and the min(t, T - 1) mask load of the 64-frame epilogue."""
    run_kind(lib, "oproj", "sat", [CC.BIG_SHAPE + (256,)])


@pytest.mark.parametrize("form", CC.FORMS)
def test_wrong_parameters_are_noticed(lib, form):
    """The comparison on the device has teeth: the taps of one channel group reversed, or two channels' BatchNorm pairs exchanged
    (what test_convmodule_cases_cpu.py plants in the model), handed to the real kernel, fail the saturated case."""
    c = CC.Case(form, "sat", 3, 65, 7)
    dw = c.dw.clone()
    dw[CC.TAPS_GROUP] = dw[CC.TAPS_GROUP].flip(1)
    msg, _ = run_case(lib, c, dw=dw)
    assert msg is not None and "wrong elements" in msg, msg
    idx = torch.arange(c.C)
    idx[list(CC.SWAP_PAIR)] = idx[list(CC.SWAP_PAIR[::-1])]
    msg, _ = run_case(lib, c, sc=c.sc[idx], sh=c.sh[idx])
    assert msg is not None and "wrong elements" in msg, msg


def test_t32_kernel_in_a_child_process():
    """The oproj tests of this file on convmodule_kernel<true>: the kernel is chosen once per process, so one fresh child with
    MINDAUDIO_AMD_CONVMOD=t32."""
    env = dict(os.environ, MINDAUDIO_AMD_CONVMOD="t32")
    args = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-k", "oproj", "-p", "no:cacheprovider"]
    res = subprocess.run(args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode(errors="replace")
    lines = re.findall(r"^\.*(convmodule_kernel<true> .*)$", out, flags=re.M)   # (pytest -q puts its progress dots in front)
    for line in lines:
        print(line)
    assert res.returncode == 0, out[-3000:]
    assert " passed" in out and "failed" not in out, out[-3000:]
    for kind in CC.KINDS:   # every kind reported at least once by the 32-frame kernel
        assert any(line.split()[1] == kind for line in lines), (kind, out[-3000:])
