"""The walking form of subsample_fused_kernel (the default of ma_subsample_fused_bf16; ma_subsample_fused_walk_bf16 bounds its grid)
against the one-tile-per-workgroup kernel, which MINDAUDIO_AMD_SUBSAMPLE=tile selects per process: the same seeded inputs run here
and, once, in a child process on the one-tile kernel, and every output agrees BIT FOR BIT - the per-tile arithmetic is the same
code, only which workgroup runs a tile, and when its prologue runs, differs.  Every output sits between sentinel rows.

T' = ((T - 3) // 2 + 1 - 3) // 2 + 1 output frames, 19 T' positions, tiles of 128:
    T = 7     1 frame, 19 positions: one partial tile
    T = 31    7 frames, 133 positions: a full tile and a tail of 5
    T = 515   128 frames, 2 432 positions: 19 full tiles exactly
    T = 1000  249 frames, 4 731 positions: 37 tiles, 123 positions in the last (the bench's utterance)
With B = 3 and max_workgroups 1, 2, 3, 5 one workgroup walks every tile, walks cross utterance boundaries, and walks of different
lengths share a launch.  Both input layouts the kernel accepts (time-fast: a transposed view of (B, 80, T + 1), as the bench passes
it; feature-fast), each with and without CMVN."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8          # sentinel rows (of 256 bf16) in front of and behind the output
SENTINEL = -21555  # 0xABCD as int16
DEFAULT = 0
# (B, T, max_workgroups values of ma_subsample_fused_walk_bf16)
SHAPES = [(1, 7, (DEFAULT, 1)), (2, 31, (DEFAULT, 1)), (1, 515, (DEFAULT, 3)), (2, 1000, (DEFAULT, 7)),
          (3, 31, (1, 2, 3, 5, DEFAULT)), (3, 1000, (1, 2, 3, 5, DEFAULT))]
CASES = [(b, tt, mws, tfast, cmvn) for (b, tt, mws) in SHAPES for tfast in (True, False) for cmvn in (True, False)]


def _key(case):
    b, tt, _, tfast, cmvn = case
    return "b%d_t%d_%s_%s" % (b, tt, "tfast" if tfast else "ffast", "cmvn" if cmvn else "raw")


def _frames(tt):
    return ((tt - 3) // 2 + 1 - 3) // 2 + 1


class _Front:
    """The weights (shared by every case) and one launch through either entry point."""

    def __init__(self):
        import torch

        from mindaudio_amd import _host, _lib, ops

        assert torch.cuda.is_available()
        self.t, self.host, self.lib = torch, _host, _lib.load()

        def r(seed, *shape, scale=1.0):
            return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()

        self.b1, self.b2 = r(2, 256, scale=0.1), r(4, 256, scale=0.1)
        self.mean = r(5, 80)
        self.istd = (torch.rand(80, generator=torch.Generator().manual_seed(6)) + 0.5).cuda()
        self.pk = ops.subsample_fused_pack(r(1, 256, 9, scale=0.3), r(3, 256, 3, 3, 256, scale=1.0 / 48).bfloat16(), 80)
        assert self.pk is not None

    def x(self, case):
        torch = self.t
        b, tt, _, tfast, _ = case
        x = torch.randn(b, tt, 80, generator=torch.Generator().manual_seed(1000 * tt + b)).cuda()
        if tfast:  # fbank's (B, n_mels, T + 1) output viewed as (B, T, n_mels)
            buf = torch.zeros(b, 80, tt + 1, device="cuda")
            buf[:, :, :tt] = x.transpose(1, 2)
            x = buf.transpose(1, 2)[:, :tt]
            assert x.stride(1) == 1 and x.stride(2) == tt + 1
        else:
            assert x.stride(2) == 1
        return x

    def run(self, case, x, max_workgroups=None):
        """-> (rc, output rows (B * 19 T', 256) as int16 or None); None: ma_subsample_fused_bf16, else the walk entry point."""
        torch = self.t
        b, tt, _, _, cmvn = case
        rows = b * _frames(tt) * 19
        buf = torch.full((GUARD + rows + GUARD, 256), SENTINEL, dtype=torch.int16, device="cuda")
        p = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
        mean, istd = (self.mean, self.istd) if cmvn else (None, None)
        args = [p(x), x.stride(0), x.stride(1), x.stride(2), b, tt, 80, p(mean), p(istd), p(self.pk), p(self.b1), p(self.b2), 256,
                ctypes.c_void_p(buf.data_ptr() + GUARD * 512)]
        if max_workgroups is None:
            rc = self.lib.ma_subsample_fused_bf16(*args, self.host.current_stream_ptr())
        else:
            rc = self.lib.ma_subsample_fused_walk_bf16(*args, max_workgroups, self.host.current_stream_ptr())
        torch.cuda.synchronize()
        if rc != 0:
            assert bool((buf == SENTINEL).all()), "a refused call wrote"
            return rc, None
        out = buf.cpu().numpy()
        assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + rows:] == SENTINEL).all(), "sentinel rows were written"
        return rc, out[GUARD:GUARD + rows]


@pytest.fixture(scope="module")
def front():
    return _Front()


@pytest.fixture(scope="module")
def want(tmp_path_factory):
    """Every case on the one-tile kernel: a fresh child process, started before this one's first launch matters to it."""
    path = str(tmp_path_factory.mktemp("tile") / "tile.npz")
    env = dict(os.environ, MINDAUDIO_AMD_SUBSAMPLE="tile")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    assert res.returncode == 0, res.stdout.decode(errors="replace")[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _same(got, ref, what):
    assert got.shape == ref.shape, what
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "%s: %d of %d elements differ, first at row %d channel %d" % (what, len(bad), got.size, bad[0][0], bad[0][1])


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_walk_matches_the_one_tile_kernel(front, want, case):
    ref = want[_key(case)]
    assert ref.shape == (case[0] * _frames(case[1]) * 19, 256)
    assert (ref != SENTINEL).all() and ref.any(), "an all-zero reference compares nothing"
    x = front.x(case)
    rc, got = front.run(case, x)  # the default of ma_subsample_fused_bf16
    assert rc == 0
    _same(got, ref, "ma_subsample_fused_bf16")
    for mw in case[2]:
        rc, got = front.run(case, x, mw)
        assert rc == 0
        _same(got, ref, "max_workgroups = %d" % mw)


def test_argument_checks(front):
    from mindaudio_amd import _lib

    case = (2, 31, (), False, True)
    x = front.x(case)
    for mw in (-1, -7, -2 ** 31):
        rc, _ = front.run(case, x, mw)
        assert rc == _lib.MA_ERR_INVALID_ARG, mw
    rc, _ = front.run((2, 6, (), False, True), x, 0)  # T < 7: no output frame
    assert rc == _lib.MA_ERR_INVALID_ARG


if __name__ == "__main__":  # the child process of `want`: every case through ma_subsample_fused_bf16 on the kernel the variable selects
    sys.path.insert(0, ROOT)
    assert os.environ.get("MINDAUDIO_AMD_SUBSAMPLE") == "tile"
    f = _Front()
    outs = {}
    for c in CASES:
        rc, out = f.run(c, f.x(c))
        assert rc == 0, (c, rc)
        outs[_key(c)] = out
    np.savez(sys.argv[1], **outs)
