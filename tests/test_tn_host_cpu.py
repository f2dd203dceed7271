"""CPU: the host side of the TN weight-gradient GEMM family (csrc/gemm_tn_bf16.hip, gemm_tn8_bf16.hip, reduce_splits.hip): launch
plans, workspace sizes and the code every entry point returns for a bad argument.  Every check of these entry points fires before
any device call, so the tables below run with small integers in place of device pointers; no row reaches a launch.  A row that
would is left out: the alignment of a pointer no entry point checks (`out`, `dw`), and a bad item behind eight good ones of
ma_gemm_tn_partial_group_bf16, whose first group is launched before the ninth item is read (that one runs on real buffers in
tests/test_train_kernels_gpu.py::test_partial_group_bad_ninth_item_leaves_first_group_issued).  The expected plans and codes are the
answers of the library as it stood before the checks, plans and split sums got one owner each."""
import pytest

from mindaudio_amd import _lib

OK, INVALID, UNSUPPORTED, WORKSPACE = _lib.MA_OK, _lib.MA_ERR_INVALID_ARG, _lib.MA_ERR_UNSUPPORTED, _lib.MA_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _build

    _build.build()
    return _lib.load()


# (Mo, No, Kc) -> (splits, workspace bytes) at 256 compute units (the MI355X's count, and what ma::num_cus() answers without a device)
_PLANS = {
    (256, 2048, 10200): (8, 16785408),
    (2048, 256, 10200): (8, 16842752),
    (64, 72, 130): (1, 18688),
    (4288, 256, 777): (1, 4408064),
    (512, 256, 577): (1, 526336),
    (8, 8, 1): (1, 288),
    (256, 256, 64): (1, 263168),
    (0, 8, 8): (-1, -1),
}


def test_tn_plans(lib):
    for shape, (splits, nbytes) in _PLANS.items():
        assert lib.ma_gemm_tn_splits(*shape) == splits, shape
        assert lib.ma_gemm_tn_workspace_bytes(*shape) == nbytes, shape
    assert lib.ma_conv2d_3x3s2_dw_workspace_bytes(193800, 256, 256) == 66088960
    assert lib.ma_conv2d_3x3s2_dw_workspace_bytes(1000, 128, 64) == 590336
    assert lib.ma_conv2d_3x3s2_dw_workspace_bytes(0, 128, 64) == INVALID


# ---- one TN product: (Kc 130, Mo 64, No 72), 40 rows stored: 1 split x 40 x (72 + 1) x 4 = 11680 bytes of partials -------------------
_TN = dict(A=16, lda=64, B=32, ldb=72, out=48, ldo=72, Mo=64, No=72, Kc=130, Mo_store=40, ws=64, ws_bytes=11680)

# (changed arguments, code) - one cause per row, then rows with two causes that pin the order in which the checks fire
_TN_ROWS = [
    (dict(A=None), INVALID), (dict(B=None), INVALID), (dict(ws=None), INVALID),
    (dict(Mo=0), INVALID), (dict(No=0), INVALID), (dict(Kc=0), INVALID), (dict(Mo_store=0), INVALID), (dict(Mo_store=65), INVALID),
    (dict(Mo=60), UNSUPPORTED), (dict(No=68), UNSUPPORTED),
    (dict(lda=65), UNSUPPORTED), (dict(lda=56), UNSUPPORTED), (dict(ldb=73), UNSUPPORTED), (dict(ldb=64), UNSUPPORTED),
    (dict(Mo=1 << 31, lda=1 << 31), UNSUPPORTED), (dict(No=1 << 31, ldb=1 << 31, ldo=1 << 31), UNSUPPORTED),
    (dict(Kc=1 << 31), UNSUPPORTED),
    (dict(A=8), INVALID), (dict(B=8), INVALID), (dict(ws=8), INVALID),
    (dict(ws_bytes=11679), WORKSPACE), (dict(ws_bytes=16), WORKSPACE),
    (dict(A=None, Mo=60), INVALID),         # null pointers before & 7
    (dict(Mo_store=65, lda=65), INVALID),   # the stored rows before the strides
    (dict(A=8, Mo=60), UNSUPPORTED),        # & 7 before the alignment
    (dict(B=8, ws_bytes=16), INVALID),      # the alignment before the plan and its workspace
]
_TN_OUT_ROWS = [(dict(out=None), INVALID), (dict(ldo=71), UNSUPPORTED), (dict(out=None, ldo=71), INVALID), (dict(ldo=71, A=8), UNSUPPORTED)]


def _tn_args(changes):
    a = dict(_TN)
    a.update(changes)
    return a


def test_gemm_tn_rejections(lib):
    for changes, code in _TN_ROWS + _TN_OUT_ROWS:
        a = _tn_args(changes)
        rc = lib.ma_gemm_tn_bf16_f32(a["A"], a["lda"], a["B"], a["ldb"], a["out"], a["ldo"], a["Mo"], a["No"], a["Kc"], a["Mo_store"],
                                     1.0, 0, None, a["ws"], a["ws_bytes"], None)
        assert rc == code, changes


def test_gemm_tn_partial_rejections(lib):
    for changes, code in _TN_ROWS:
        for with_colsum in (0, 1):
            a = _tn_args(changes)
            rc = lib.ma_gemm_tn_partial_bf16(a["A"], a["lda"], a["B"], a["ldb"], a["Mo"], a["No"], a["Kc"], a["Mo_store"], with_colsum,
                                             a["ws"], a["ws_bytes"], None)
            assert rc == code, changes


def _tn_item(it, a):
    it.A, it.B, it.partial, it.lda, it.ldb = a["A"], a["B"], a["ws"], a["lda"], a["ldb"]
    it.Mo, it.No, it.Kc, it.Mo_store, it.partial_bytes, it.with_colsum = a["Mo"], a["No"], a["Kc"], a["Mo_store"], a["ws_bytes"], 1


def test_gemm_tn_partial_group_rejections(lib):
    """The bad item comes first: the entry point validates and launches per group of eight, so nothing has been launched when it
    answers - alone, in front of two good items, and in front of eight (a second group that is never reached)."""
    one = (_lib.TnItem * 1)()
    assert lib.ma_gemm_tn_partial_group_bf16(None, 1, None) == INVALID
    _tn_item(one[0], _TN)
    assert lib.ma_gemm_tn_partial_group_bf16(one, 0, None) == INVALID
    for n in (1, 3, 9):
        items = (_lib.TnItem * n)()
        for changes, code in _TN_ROWS:
            for k in range(n):
                _tn_item(items[k], _tn_args(changes) if k == 0 else _TN)
            assert lib.ma_gemm_tn_partial_group_bf16(items, n, None) == code, (n, changes)


# ---- the 256 x 256-tile products without split-K ------------------------------------------------------------------------------------
_DIRECT = dict(A=16, B=32, out=48, lda=256, ldb=512, ldo=512, Mo=256, No=512, Kc=65)
_DIRECT_ROWS = [
    dict(A=None), dict(B=None), dict(out=None), dict(Kc=0), dict(Mo=0), dict(No=0),
    dict(Mo=264, lda=264), dict(Mo=128), dict(No=520, ldb=520, ldo=520), dict(No=128),
    dict(lda=257), dict(lda=248), dict(ldb=513), dict(ldb=504), dict(ldo=514), dict(ldo=508),
    dict(lda=1 << 31), dict(ldb=1 << 31), dict(ldo=1 << 31),
    dict(A=8), dict(B=8), dict(out=8),
]


def _direct_item(it, changes=()):
    a = dict(_DIRECT)
    a.update(changes)
    it.A, it.B, it.out, it.colsum = a["A"], a["B"], a["out"], None
    it.lda, it.ldb, it.ldo, it.Mo, it.No, it.Kc = a["lda"], a["ldb"], a["ldo"], a["Mo"], a["No"], a["Kc"]


def test_gemm_tn_direct_group_rejections(lib):
    """Every item is validated before the one launch, so the bad item may stand anywhere: first, ninth, last."""
    cap = lib.ma_gemm_tn_direct_max_items()
    assert cap == 56
    items = (_lib.TnDirectItem * (cap + 1))()
    for it in items:
        _direct_item(it)
    assert lib.ma_gemm_tn_direct_group_bf16(None, 1, None) == INVALID
    assert lib.ma_gemm_tn_direct_group_bf16(items, 0, None) == INVALID
    assert lib.ma_gemm_tn_direct_group_bf16(items, cap + 1, None) == INVALID
    for changes in _DIRECT_ROWS:
        for bad, n in ((0, 1), (0, 3), (8, 9), (cap - 1, cap)):
            _direct_item(items[bad], changes)
            assert lib.ma_gemm_tn_direct_group_bf16(items, n, None) == UNSUPPORTED, (changes, bad, n)
            _direct_item(items[bad])
    _direct_item(items[cap], dict(A=None))  # (n counts before any item is read)
    assert lib.ma_gemm_tn_direct_group_bf16(items, cap + 1, None) == INVALID


# ---- the conv2 weight gradient ------------------------------------------------------------------------------------------------------
def _dw(lib, a):
    return lib.ma_conv2d_3x3s2_dw_bf16(a["dy"], a["ld_dy"], a["act"], a["batch"], a["H"], a["Wd"], a["C"], a["Cout"], a["dw"], None,
                                       a["ws"], a["ws_bytes"], None)


def test_conv2d_dw_rejections(lib):
    # the 128-tile im2col route: batch 2, 9 x 11 -> 4 x 5 outputs, M = 40 rows
    small = dict(dy=16, ld_dy=64, act=32, batch=2, H=9, Wd=11, C=128, Cout=64, dw=48, ws=64)
    small["ws_bytes"] = lib.ma_conv2d_3x3s2_dw_workspace_bytes(40, 128, 64)
    assert small["ws_bytes"] == lib.ma_gemm_tn_workspace_bytes(64, 9 * 128, 40) == 295168
    rows = [
        (dict(dy=None), INVALID), (dict(act=None), INVALID), (dict(dw=None), INVALID), (dict(ws=None), INVALID),
        (dict(batch=0), INVALID), (dict(H=2), INVALID), (dict(Wd=2), INVALID), (dict(C=0), INVALID), (dict(Cout=4), INVALID),
        (dict(C=64), UNSUPPORTED), (dict(C=192), UNSUPPORTED), (dict(Cout=60), UNSUPPORTED),
        (dict(ld_dy=65), UNSUPPORTED), (dict(ld_dy=68), UNSUPPORTED), (dict(ld_dy=56), UNSUPPORTED),
        (dict(batch=838861), UNSUPPORTED),  # x 20 outputs = 16 777 220 rows >= 2^24
        (dict(ws_bytes=small["ws_bytes"] - 1), WORKSPACE), (dict(ws_bytes=16), WORKSPACE),
        (dict(dy=None, C=64), INVALID), (dict(H=2, ld_dy=65), INVALID), (dict(C=64, batch=838861), UNSUPPORTED),
        (dict(batch=838861, ws_bytes=16), UNSUPPORTED),
    ]
    for changes, code in rows:
        a = dict(small)
        a.update(changes)
        assert _dw(lib, a) == code, changes
    # the 256-tile route: batch 4, 65 x 33 -> 32 x 16 outputs, M = 2048 rows, 2 splits; its launcher checks the alignment
    big = dict(dy=16, ld_dy=256, act=32, batch=4, H=65, Wd=33, C=256, Cout=256, dw=48, ws=64)
    tn8_bytes = 2 * 256 * (9 * 256 + 1) * 4
    tn_bytes = lib.ma_gemm_tn_workspace_bytes(256, 9 * 256, 2048)
    big["ws_bytes"] = lib.ma_conv2d_3x3s2_dw_workspace_bytes(2048, 256, 256)
    assert big["ws_bytes"] == max(tn8_bytes, tn_bytes)
    rows = [
        (dict(dy=8), INVALID), (dict(act=8), INVALID), (dict(ws=8), INVALID),
        (dict(ws_bytes=min(tn8_bytes, tn_bytes) - 1), WORKSPACE),  # too small for either route
        (dict(dy=None), INVALID), (dict(ld_dy=260), UNSUPPORTED), (dict(ld_dy=248), UNSUPPORTED), (dict(Cout=260, ld_dy=264), UNSUPPORTED),
    ]
    for changes, code in rows:
        a = dict(big)
        a.update(changes)
        assert _dw(lib, a) == code, changes


def test_reduce_splits_batch_rejections(lib):
    assert lib.ma_reduce_splits_batch_f32(None, 32, 1, None) == INVALID
    assert lib.ma_reduce_splits_batch_f32(16, None, 1, None) == INVALID
    assert lib.ma_reduce_splits_batch_f32(16, 32, 0, None) == INVALID
    assert lib.ma_reduce_splits_batch_f32(16, 32, -1, None) == INVALID
