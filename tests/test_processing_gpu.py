"""GPU: data.processing trim / split / trim_batch / split_batch / frame_power_device, normalize, stereo_to_mono (csrc/silence.hip)
and the indexing functions against the fixtures tests/golden/gen_processing_goldens.py recorded from the reference's own functions.

Silence.  The generator asserted that every frame's decibel value lies at least 1e-6 dB from -top_db (the smallest margin the
fixtures keep is stored: 0.517 dB), far above any float64 reordering error, so flags, trim indices and split intervals must equal
the reference's exactly, for every case.  Power rows are held to (frame_length + 4) * 2^-53 relative per frame: a sum of n
non-negative terms in another order differs by at most (n - 1) * 2^-53, the division by n and the square root and square add the
rest.  Derived, not measured.
normalize.  max, min, l0 and what is built from them only: bit for bit.  The summed statistics: 16 x max(spread, 2^-44) over the
peak, spread being the recorded difference between the reference's own result under NumPy's, a reversed and math.fsum's summation.
stereo_to_mono and the indexing functions: exact.  Repeated runs, NumPy and tensor input, a row alone and inside a ragged batch are
compared bit for bit, and every input is checked to be left as it was.

Measured on an MI355X: the ERRTABLE in DESIGN.md 8.2.3."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import processing_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR64 = 2.0 ** -44


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


def _kw(c):
    return dict(top_db=c["top_db"], reference=C.reference_arg(c), frame_length=c["frame_length"], hop_length=c["hop_length"])


def _power_check(tag, power, ref, frame_length):
    bound = (frame_length + 4) * 2.0 ** -53
    rel = np.abs(power - ref) / np.where(ref > 0, ref, 1.0)
    assert np.all(power[ref == 0] == 0)
    print("ERRTABLE power %s frames %d bound %.3g gpu %.3g" % (tag, len(ref), bound, rel.max()))
    assert rel.max() <= bound, (tag, rel.max(), bound)
    return rel.max()


@pytest.mark.parametrize("case", list(C.SILENCE_CASES))
def test_trim_and_split_against_the_reference(torch, fix, case):
    from mindaudio_amd.data import processing as P

    c = C.SILENCE_CASES[case]
    x = fix[case + "/x"]
    keep = x.copy()
    xt = torch.from_numpy(x).cuda()
    # the power row and the flags, through the device entries the public functions are made of
    mono = P.stereo_to_mono(xt) if x.ndim > 1 else xt
    power, row_max = P.frame_power_device(mono.reshape(1, -1), None, c["frame_length"], c["hop_length"])
    assert power.dtype == torch.float64 and tuple(power.shape) == (1, len(fix[case + "/power"]))
    _power_check(case, power[0].cpu().numpy(), fix[case + "/power"], c["frame_length"])
    assert float(row_max[0]) == float(power[0].max())
    flags = P.silence_edges_device(power, row_max, mono.numel(), None, c["frame_length"], c["hop_length"], c["top_db"],
                                   C.reference_arg(c))[0]
    assert np.array_equal(flags[0].cpu().numpy().astype(bool), fix[case + "/flags"])
    # trim
    for inp in (x, xt):
        if case + "/trim_error" in fix.files:
            with pytest.raises(IndexError):
                P.trim(inp, **_kw(c))
            continue
        trimmed, index = P.trim(inp, **_kw(c))
        assert isinstance(index, np.ndarray) and index.dtype.kind == "i" and np.array_equal(index, fix[case + "/trim_index"])
        assert isinstance(trimmed, type(inp))
        got = trimmed.cpu().numpy() if inp is xt else trimmed
        assert got.dtype == x.dtype and np.array_equal(got, x[index[0]:index[1]])
    # split
    for inp in (x, xt):
        intervals = P.split(inp, **_kw(c))
        assert isinstance(intervals, np.ndarray) and intervals.dtype.kind == "i" and intervals.ndim == 2 and intervals.shape[1] == 2
        assert np.array_equal(intervals, fix[case + "/split"]), (intervals, fix[case + "/split"])
    assert np.array_equal(x, keep) and torch.equal(xt.cpu(), torch.from_numpy(keep))
    if c["reference"] == "max":  # any other callable sees the power row on the host: np.amax spelled as a lambda
        assert np.array_equal(P.split(x, **dict(_kw(c), reference=lambda p: p.max())), fix[case + "/split"])


def test_the_reference_quirks_are_kept(torch, fix):
    from mindaudio_amd.data import processing as P

    trimmed, index = P.trim(fix["doc_trim/x"], top_db=10)
    assert list(index) == [512, 3072] and trimmed.shape == (2488,)  # the end is not clipped to 3000; the slice is
    assert np.array_equal(P.split(fix["doc_split/x"], top_db=10), [[1536, 5120], [5632, 8192]])
    ch3 = P.split(fix["ch3_float32/x"], **_kw(C.SILENCE_CASES["ch3_float32"]))
    assert np.array_equal(ch3, fix["ch3_float32/split"]) and ch3.max() == 3  # clipped with shape[-1]: the channel count
    assert fix["zeros/flags"].all() and np.array_equal(P.split(fix["zeros/x"], frame_length=64, hop_length=16), [[0, 199]])
    with pytest.raises(ValueError):
        P.trim(fix["zeros/x"], hop_length=0)


@pytest.mark.parametrize("name", list(C.batches()))
def test_batched_entries_equal_the_rows_alone(torch, fix, name):
    from mindaudio_amd.data import processing as P

    fl, hop, rows = C.batches()[name]
    lengths = [C.SILENCE_CASES[r]["shape"][0] for r in rows]
    T = max(lengths)
    batch = np.full((len(rows), T), 0.25, np.float32)  # what lies behind a row's length must not count
    for b, r in enumerate(rows):
        batch[b, :lengths[b]] = fix[r + "/x"]
    for dtype in (torch.float32, torch.float64):
        xt = torch.from_numpy(batch).cuda().to(dtype)
        keep = xt.clone()
        lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        power, row_max = P.frame_power_device(xt, lens, fl, hop)
        index = P.trim_batch(xt, lengths, top_db=60, frame_length=fl, hop_length=hop)
        counts, edges = P.split_batch(xt, lens, top_db=60, frame_length=fl, hop_length=hop)
        assert index.is_cuda and index.dtype == torch.int32 and tuple(index.shape) == (len(rows), 2)
        assert counts.is_cuda and edges.is_cuda and tuple(edges.shape) == (len(rows), power.shape[1] + 1)
        assert torch.equal(P.frame_power_device(xt, lens, fl, hop)[0], power)  # two runs: the same bits
        assert torch.equal(P.split_batch(xt, lens, top_db=60, frame_length=fl, hop_length=hop)[1], edges)
        for b, r in enumerate(rows):
            F = len(fix[r + "/power"])
            _power_check("%s[%d]" % (name, b), power[b, :F].cpu().numpy(), fix[r + "/power"], fl)
            assert bool((power[b, F:] == 0).all())
            alone = P.frame_power_device(xt[b:b + 1, :lengths[b]].contiguous(), None, fl, hop)
            assert torch.equal(alone[0][0], power[b, :F]) and torch.equal(alone[1][0], row_max[b])  # alone: the same bits
            assert np.array_equal(index[b].cpu().numpy(), fix[r + "/trim_index"])
            m = int(counts[b])
            assert np.array_equal(edges[b, :2 * m].cpu().numpy().reshape(-1, 2), fix[r + "/split"])
            assert bool((edges[b, 2 * m:] == -1).all())
        assert torch.equal(xt, keep)
    if len(rows) == 1:  # lengths=None: every row is T long
        assert np.array_equal(P.trim_batch(xt, None, frame_length=fl, hop_length=hop)[0].cpu().numpy(), fix[rows[0] + "/trim_index"])


def test_batched_scalar_reference_and_the_sentinel(torch, fix):
    from mindaudio_amd.data import processing as P

    names = ["ref_1_60", "ref_none_pass", "ref_001_10"]
    xt = torch.from_numpy(np.stack([fix[k + "/x"] for k in names])).cuda()
    for k, (ref, db) in enumerate(((1.0, 60), (100.0, 10), (0.01, 10))):
        index = P.trim_batch(xt, None, top_db=db, reference=ref, frame_length=64, hop_length=16).cpu().numpy()
        counts, edges = P.split_batch(xt, None, top_db=db, reference=ref, frame_length=64, hop_length=16)
        if names[k] == C.NONE_PASS_CASE:
            assert np.array_equal(index, np.full((3, 2), -1)) and int(counts.sum()) == 0 and bool((edges == -1).all())
        else:
            assert np.array_equal(index[k], fix[names[k] + "/trim_index"])
            assert np.array_equal(edges[k, :2 * int(counts[k])].cpu().numpy().reshape(-1, 2), fix[names[k] + "/split"])
    per_row = torch.tensor([1.0, 100.0, 0.01], dtype=torch.float64, device="cuda")  # a reference per row, on the device
    index = P.trim_batch(xt, None, top_db=10, reference=per_row, frame_length=64, hop_length=16).cpu().numpy()
    assert list(index[1]) == [-1, -1] and np.array_equal(index[2], fix["ref_001_10/trim_index"])


def _norm_cases():
    return sorted({(name, axis) for name, axis, _, _ in C.normalize_cases()})


@pytest.mark.parametrize("name,axis", _norm_cases())
def test_normalize_against_the_reference(torch, fix, name, axis):
    from mindaudio_amd.data import processing as P

    x64 = fix["norm/%s/x" % name]
    pos = C.kept(x64.shape)
    for dtype in C.NORM_DTYPES:
        x = C.cast(x64, dtype)
        keep = x.copy()
        xt = torch.from_numpy(x).cuda()
        for norm in C.NORMS:
            key = C.norm_key(name, axis, norm, dtype)
            ref = fix[key]
            y = P.normalize(x, norm=norm, axis=axis)
            assert isinstance(y, np.ndarray) and y.shape == x.shape and y.dtype == ref.dtype, (key, y.dtype, ref.dtype)
            yt = P.normalize(xt, norm=norm, axis=axis - x.ndim)  # the same axis, counted from the end
            assert yt.is_cuda and np.array_equal(yt.cpu().numpy(), y, equal_nan=True)
            assert np.array_equal(P.normalize(x, norm=norm, axis=axis), y, equal_nan=True)  # two runs
            got = y.reshape(-1)[pos]
            if norm in C.EXACT_NORMS:
                assert np.array_equal(got, ref), key
            else:
                spread = float(fix[key + "/spread"])
                e = C.peak_error(got, ref)
                print("ERRTABLE normalize %s spread %.3g gpu %.3g" % (key, spread, e))
                assert e <= 16 * max(spread, FLOOR64), (key, e, spread)
        assert np.array_equal(x, keep) and torch.equal(xt.cpu(), torch.from_numpy(keep))


def test_normalize_over_all_of_the_array_and_its_refusals(torch, fix):
    from mindaudio_amd.data import processing as P

    x = fix["norm/m4x3/x"]
    assert np.array_equal(P.normalize(x, norm="max", axis=None), x / np.abs(x).max())
    with pytest.raises(TypeError):
        P.normalize(x, norm="l3")
    with pytest.raises(NotImplementedError):
        P.normalize(x.astype(np.complex64))
    with pytest.raises(ValueError):
        P.normalize(x, axis=2)
    small = np.array([[3, 0, 250], [1, 0, 5]], np.uint8)  # the small integer types go through the kernel as int64
    y = P.normalize(small, norm="max", axis=1)
    assert y.dtype == np.uint8 and np.array_equal(y, [[0, 0, 1], [0, 0, 1]])


@pytest.mark.parametrize("name", list(C.MONO_CASES))
def test_stereo_to_mono_bit_for_bit(torch, fix, name):
    from mindaudio_amd.data import processing as P

    x, ref = fix[name + "/x"], fix[name + "/out"]
    keep = x.copy()
    if x.ndim == 1:
        assert P.stereo_to_mono(x) is x
        xt = torch.from_numpy(x).cuda()
        assert P.stereo_to_mono(xt) is xt
        return
    y = P.stereo_to_mono(x)
    assert isinstance(y, np.ndarray) and y.dtype == ref.dtype and y.shape == ref.shape
    assert np.array_equal(y.view(np.uint8), ref.view(np.uint8)), name
    yt = P.stereo_to_mono(torch.from_numpy(x).cuda())
    assert yt.is_cuda and np.array_equal(yt.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    assert np.array_equal(x, keep)
    if x.dtype == np.float32 and x.shape[1] == 3:
        with pytest.raises(NotImplementedError):
            P.stereo_to_mono(np.zeros((4, 9), np.float32))
        batch = np.stack([x, -x])  # (2, n, 3): the mean over the last axis, whatever lies in front
        assert np.array_equal(P.stereo_to_mono(batch), np.mean(batch, axis=-1))
        assert np.array_equal(P.stereo_to_mono(x.astype(np.int64)), np.mean(x.astype(np.int64), axis=-1))


@pytest.mark.parametrize("name", list(C.INDEX_CASES))
def test_indexing_functions_exactly(torch, fix, name):
    from mindaudio_amd.data import processing as P

    fn, args = C.INDEX_CASES[name]
    ref, printed = fix[name + "/out"], str(fix[name + "/printed"])
    args = [fix["%s/arg%d" % (name, k)] if isinstance(a, np.ndarray) else a for k, a in enumerate(args)]
    keep = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
    for device in (False, True):
        call = [torch.from_numpy(a).cuda() if device and isinstance(a, np.ndarray) else a for a in args]
        with contextlib.redirect_stdout(io.StringIO()) as said:
            y = getattr(P, fn)(*call)
        assert said.getvalue() == printed
        if device:
            assert isinstance(y, torch.Tensor) and y.is_cuda
            for a, k in zip(call, keep):
                if isinstance(k, np.ndarray):
                    assert torch.equal(a.cpu(), torch.from_numpy(k))
            y = y.cpu().numpy()
        assert isinstance(y, np.ndarray) and y.dtype == ref.dtype and y.shape == ref.shape and np.array_equal(y, ref), name
    for a, k in zip(args, keep):
        if isinstance(k, np.ndarray):
            assert np.array_equal(a, k)  # invert_channels too: the one departure from the reference


def test_entry_points_reject_bad_arguments_and_launch_nothing(torch):
    from mindaudio_amd import _lib

    lib = _lib.load()
    x = torch.zeros((2, 100), device="cuda")
    power = torch.full((2, 7), 7.0, dtype=torch.float64, device="cuda")
    row_max = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((2, 7), 7, dtype=torch.uint8, device="cuda")
    index = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    edges = torch.full((2, 8), 7, dtype=torch.int32, device="cuda")
    P, null = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)

    def fp(x=P(x), sample_bytes=4, B=2, T=100, ldx=100, fl=64, hop=16, power=P(power), ldp=7, row_max=P(row_max)):
        return lib.ma_frame_power(x, sample_bytes, B, T, ldx, null, fl, hop, power, ldp, row_max, null)

    def se(power=P(power), ldp=7, B=2, T=100, fl=64, hop=16, flags=P(flags), index=P(index), counts=P(counts), edges=P(edges)):
        return lib.ma_silence_edges(power, ldp, B, T, null, fl, hop, null, 1e-10, 60.0, -1, flags, index, counts, edges, null)

    for bad in (dict(x=null), dict(power=null), dict(row_max=null), dict(sample_bytes=2), dict(B=0), dict(T=0), dict(fl=0), dict(hop=0),
                dict(ldx=99), dict(ldp=6)):
        assert fp(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    for bad in (dict(power=null), dict(flags=null), dict(index=null), dict(counts=null), dict(edges=null), dict(B=0), dict(T=0),
                dict(fl=0), dict(hop=0), dict(ldp=6)):
        assert se(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    out = torch.full((100,), 7.0, dtype=torch.float64, device="cuda")
    assert lib.ma_axis_stats(P(x), 9, 2, 100, 1, 0, P(out), null) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_axis_stats(P(x), 0, 2, 100, 1, 7, P(out), null) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_axis_stats(P(x), 0, 2, 0, 1, 0, P(out), null) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_axis_apply(P(x), 0, 2, 100, 1, null, null, P(out), 1, null) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_axis_apply(P(x), 0, 1, 100, 1, P(row_max), null, P(out), 3, null) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_channel_mean(P(x), 4, 20, 9, P(out), null) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_channel_mean(P(x), 4, 0, 2, P(out), null) == _lib.MA_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for t in (power, row_max, flags, index, counts, edges, out):
        assert bool((t == 7).all())  # nothing was launched
    assert fp() == _lib.MA_OK and se() == _lib.MA_OK  # an all-zero input: every frame at the floor, one interval per row
    torch.cuda.synchronize()
    assert bool((power == 0).all()) and bool((flags == 1).all()) and index.cpu().tolist() == [[0, 112], [0, 112]]
    assert counts.cpu().tolist() == [1, 1] and edges.cpu()[:, :3].tolist() == [[0, 100, -1], [0, 100, -1]]
