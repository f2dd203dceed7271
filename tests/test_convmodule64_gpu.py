"""The 64-frame conv-module launch (convmodule64_kernel, the default form of ma_attn_out_convmodule_bf16) against the 32-frame
kernel it replaced, which MINDAUDIO_AMD_CONVMOD=t32 selects per process: the same cases run here and in a child process on t32, and
the outputs agree within the per-element bound test_conformer_ops_gpu.py::test_attn_out_convmodule_one_launch uses for its large case
(the LayerNorm row sums are reduced in another order, so a few bf16 elements of a = LN(x') may round the other way; nothing larger)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, T, k, masked): the bench shape, the shapes of test_attn_out_convmodule_one_launch, then seeded random ones - T < 64,
# T = 1 mod 64 (a last tile of one frame), single-tile utterances, every odd k
CASES = [(64, 249, 15, True), (3, 249, 15, True), (2, 33, 7, True), (5, 64, 15, False), (1, 5, 3, True), (2, 32, 15, False),
         (150, 224, 15, True), (4, 65, 15, True), (3, 129, 9, False), (2, 193, 15, True), (7, 1, 15, True), (5, 63, 1, True)]
_rng = np.random.RandomState(64)
for _ in range(8):
    CASES.append((int(_rng.randint(1, 13)), int(_rng.randint(2, 400)), int(2 * _rng.randint(0, 8) + 1), bool(_rng.rand() < 0.7)))


def _case_outputs(cases):
    import torch

    from mindaudio_amd import ops

    def r(seed, *shape, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()

    outs = {}
    c = 256
    for i, (b, tt, ks, masked) in enumerate(cases):
        s = 1000 * i
        ctx = r(s + 1, b * tt, c).bfloat16()
        po = ops.gemm_k256_pack(r(s + 2, c, c, scale=1.0 / 16).bfloat16())
        p1 = ops.gemm_k256_pack(r(s + 3, 2 * c, c, scale=1.0 / 16).bfloat16())
        p2 = ops.gemm_k256_pack(r(s + 4, c, c, scale=1.0 / 16).bfloat16())
        bo, b1, b2 = r(s + 5, c, scale=0.2), r(s + 6, 2 * c, scale=0.2), r(s + 7, c)
        lg, lb = 1 + 0.1 * r(s + 8, c), 0.1 * r(s + 9, c)
        dw = r(s + 10, c, ks, scale=0.3)
        sc, sh = 1 + 0.1 * r(s + 11, c), 0.1 * r(s + 12, c)
        x = r(s + 13, b * tt, c)
        mask = (torch.rand(b * tt, generator=torch.Generator().manual_seed(s + 14)) > 0.2).float().cuda() if masked else None
        x0 = x.clone()
        got = ops.attn_out_convmodule(ctx, po, bo, lg, lb, p1, b1, dw, sc, sh, p2, b2, mask, x, b, tt,
                                      out=torch.full_like(x, float("nan")))
        again = ops.attn_out_convmodule(ctx, po, bo, lg, lb, p1, b1, dw, sc, sh, p2, b2, mask, x, b, tt)
        assert torch.equal(x, x0), "x was written"
        assert torch.equal(got, again), "not deterministic"
        outs["c%d" % i] = got.cpu().numpy()
    return outs


def _child(env_value, args):
    env = dict(os.environ, MINDAUDIO_AMD_CONVMOD=env_value)
    res = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = res.stdout.decode(errors="replace")
    assert res.returncode == 0, out[-3000:]
    return out


def test_convmodule64_matches_the_32_frame_kernel(tmp_path):
    import torch

    assert torch.cuda.is_available()
    path = str(tmp_path / "t32.npz")
    _child("t32", [os.path.abspath(__file__), path])
    want = np.load(path)
    got = _case_outputs(CASES)
    for i, case in enumerate(CASES):
        g, w = got["c%d" % i], want["c%d" % i]
        assert np.isfinite(g).all(), case
        d, top = np.abs(g - w), float(np.abs(w).max())
        # the LayerNorm sums are reduced in the 32-frame kernel's order, so the outputs match bit for bit (the bench shape does);
        # the bound is what a flipped element of a would cost: one bf16 step of a in the rows that convolve it, within 1e-3 of the
        # scale as the large case of test_attn_out_convmodule_one_launch allows.  How many elements such flips move depends on the
        # data: on these cases the 32-frame kernel and the two-launch path (gemm_packed_ln + convmodule) differ in up to 1.2 %.
        assert float(d.max()) <= 1e-3 * top, (case, float(d.max()), top)
        assert int((d > 1e-5 * top).sum()) <= 2e-2 * d.size, case


def test_32_frame_fallback_still_passes():
    out = _child("t32", ["-m", "pytest", os.path.join(ROOT, "tests", "test_conformer_ops_gpu.py"), "-q", "-x", "-k",
                         "attn_out_convmodule", "-p", "no:cacheprovider"])
    assert " passed" in out and "failed" not in out


if __name__ == "__main__":  # child process of the first test: the same cases on the kernel MINDAUDIO_AMD_CONVMOD selects
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **_case_outputs(CASES))
