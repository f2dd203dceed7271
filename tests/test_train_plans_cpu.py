"""The host-side owners of the training step's cached state (train/plans.py, train/block_table.py) and the engine's attribute
discipline.  No launches: torch CPU tensors stand in for device memory, a small class for BlockTable."""
import ast
import ctypes
import os
import warnings

import pytest
import torch

from mindaudio_amd import _lib
from mindaudio_amd.train.block_table import RECORD, REPLAY, SEEN, WALK, BlockTables
from mindaudio_amd.train.plans import ItemTable, PlanCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- item table --------------------------------------------------------------------------------------------------------------
def _items(kind):
    if kind is _lib.ReduceItem:
        return [_lib.ReduceItem(0x1000 * (i + 1), 0x2000 * (i + 1), 512 + i, 512, 512, 3 + i, 1.0, 3, 77, 512) for i in range(3)]
    if kind is _lib.TransposeItem:
        return [_lib.TransposeItem(0x1000 * (i + 1), 0x2000 * (i + 1), 256, 320, 300 + i, 256, 77, 4) for i in range(3)]
    return [_lib.PackItem(0x1000 * (i + 1), 0x2000 * (i + 1), 256, 2048, 256, i, 77) for i in range(3)]


@pytest.mark.parametrize("kind", [_lib.ReduceItem, _lib.TransposeItem, _lib.PackItem])
def test_item_table_uploads_the_packed_structs_the_map_and_the_grid_size(kind):
    items, counts = _items(kind), (3, 1, 2)
    table = ItemTable(zip(items, counts), "cpu")
    want = _items(kind)
    for item, first in zip(want, (0, 3, 4)):
        item.first_block = first
    assert table.items.dtype == torch.uint8 and bytes(table.items.numpy()) == bytes((kind * 3)(*want))
    assert len(bytes(table.items.numpy())) == 3 * ctypes.sizeof(kind)
    assert table.block_item.dtype == torch.int32 and table.block_item.tolist() == [0, 0, 0, 1, 2, 2]
    assert table.n_blocks == 6
    assert table.args == (table.items.data_ptr(), table.block_item.data_ptr(), 6)


def test_item_table_reduce_issues_the_batched_sum_with_its_triple(monkeypatch):
    from types import SimpleNamespace

    from mindaudio_amd import _host

    table, seen = ItemTable(zip(_items(_lib.ReduceItem), (3, 1, 2)), "cpu"), []
    monkeypatch.setattr(_lib, "load", lambda: SimpleNamespace(ma_reduce_splits_batch_f32=lambda *a: seen.append(a) or 0))
    prev = _host.swap_pinned(ctypes.c_void_p(0))
    try:
        table.reduce("sums")
        assert len(seen) == 1 and seen[0][:3] == table.args and len(seen[0]) == 4
        monkeypatch.setattr(_lib, "load", lambda: SimpleNamespace(ma_reduce_splits_batch_f32=lambda *a: _lib.MA_ERR_INVALID_ARG,
                                                                  ma_status_string=lambda rc: b"invalid argument"))
        with pytest.raises(ValueError, match="sums: invalid argument"):
            table.reduce("sums")
    finally:
        _host.swap_pinned(prev)


# ---- plan cache --------------------------------------------------------------------------------------------------------------
class _Plan:
    def __init__(self, arena):
        self.arena = arena


GROWTH = {"block sums": lambda need, old: need,
          "front": lambda need, old: max(need, int(1.25 * old)),
          "decoder LayerNorm": lambda need, old: max(need, 2 * old)}


def test_plan_cache_hit_touch_and_bound():
    dropped = []
    cache = PlanCache(3, GROWTH["front"], torch.uint8, "cpu", on_drop=dropped.append)
    arena = cache.arena_for(100)
    plans = {k: cache.put(k, _Plan(arena)) for k in "abc"}
    assert cache.get("zzz") is None and list(cache.plans) == ["a", "b", "c"]
    assert cache.get("a") is plans["a"] and list(cache.plans) == ["b", "c", "a"]  # (the identical object, most recently used last)
    assert cache.arena_for(100) is arena and cache.arena_for(7) is arena and not dropped  # (a request that fits: the same arena)
    plans["d"] = cache.put("d", _Plan(arena))
    assert dropped == [plans["b"]] and list(cache.plans) == ["c", "a", "d"] and len(cache.plans) == 3


@pytest.mark.parametrize("rule", sorted(GROWTH))
def test_plan_cache_growth_follows_the_rule_given_and_drops_every_earlier_plan(rule):
    old = 1000
    want = {"block sums": (old + 1, 3 * old), "front": (int(1.25 * old), 3 * old), "decoder LayerNorm": (2 * old, 3 * old)}[rule]
    for need, size in zip((old + 1, 3 * old), want):
        dropped = []
        cache = PlanCache(8, GROWTH[rule], torch.float32 if rule == "decoder LayerNorm" else torch.uint8, "cpu", on_drop=dropped.append)
        first = cache.arena_for(old)
        assert first.numel() == old and first.dtype == (torch.float32 if rule == "decoder LayerNorm" else torch.uint8)
        earlier = [cache.put(k, _Plan(first)) for k in range(3)]
        grown = cache.arena_for(need)
        assert grown is not first and grown.numel() == size
        assert dropped == earlier and len(cache.plans) == 0  # (each exactly once)
        cache.put("new", _Plan(grown))
        assert all(p.arena is grown for p in cache.plans.values()) and cache.arena is grown


# ---- the tables' owner -------------------------------------------------------------------------------------------------------
class _Table:
    """What the owner uses of a BlockTable."""

    made = []

    def __init__(self, nbytes=100, broken=None):
        self.size, self.broken, self.recorded, self.cleared = nbytes, broken, 0, 0
        _Table.made.append(self)

    def nbytes(self):
        return self.size

    def clear(self):
        self.cleared += 1


class _ShapePlan:
    def __init__(self):
        self.tables, self.table = {}, None


DIMS = (8, 2, "cpu")  # d, L, device of the boundary buffers


def _key(b=3, t2=5, att=None, extra=0):
    return (b, t2, att or (b, t2), extra)


def _owner(**kw):
    args = dict(max_bytes=1 << 40, min_sightings=2, max_blocks=64, make_table=_Table)
    args.update(kw)
    return BlockTables(**args)


def _bn():
    return [(torch.full((4,), 1.0), torch.full((4,), 2.0))]


def test_second_sighting_enters_recording_with_buffers_and_a_snapshot():
    own, plan, bn = _owner(), _ShapePlan(), _bn()
    assert own.entry_for(plan, _key(), 7, DIMS, bn) is None and plan.table.state == SEEN and own.recording is None
    tb = own.entry_for(plan, _key(), 7, DIMS, bn)
    assert tb is plan.table and tb.state == RECORD and own.recording is tb and isinstance(tb.table, _Table)
    assert tuple(tb.x_in.shape) == (15, 8) and tb.x_in.dtype == torch.float32 and tb.a_in.dtype == torch.bfloat16
    assert tuple(tb.mask_rows.shape) == (15,) and tuple(tb.att_mask.shape) == (3, 5) and tuple(tb.pos_all.shape) == (5, 16)
    assert tuple(tb.g.shape) == (15, 8)
    bn[0][0].fill_(9.0)  # (the snapshot is a copy, not the running statistics themselves)
    assert torch.equal(own.bn_snapshot[0][0], torch.full((4,), 1.0)) and torch.equal(own.bn_snapshot[0][1], torch.full((4,), 2.0))
    own.recorded(tb)
    assert tb.state == REPLAY and own.recording is None and own.bytes == {tb: 100}
    assert own.entry_for(plan, _key(), 7, DIMS, bn) is tb and tb.state == REPLAY
    # a higher threshold: the third sighting
    own3, plan3 = _owner(min_sightings=3), _ShapePlan()
    assert [own3.entry_for(plan3, _key(), 7, DIMS, bn) is None for _ in range(3)] == [True, True, False]


def test_more_segments_than_the_table_holds_is_walked_for_good_with_one_warning():
    own, bn = _owner(max_blocks=6), _bn()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for plan in (_ShapePlan(), _ShapePlan()):
            for _ in range(4):
                assert own.entry_for(plan, _key(), 7, DIMS, bn) is None
            assert plan.table.state == WALK and plan.table.table is None
    assert len([w for w in caught if "launch segments" in str(w.message)]) == 1 and own.recording is None and not own.bytes


def test_a_broken_recording_is_walked_for_good_and_its_entry_cleared():
    own, plan, bn = _owner(), _ShapePlan(), _bn()
    own.entry_for(plan, _key(), 7, DIMS, bn)
    tb = own.entry_for(plan, _key(), 7, DIMS, bn)
    table = tb.table
    table.broken = "ma_fft_pow2_c32 cannot be replayed from a block table"
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        own.recorded(tb)
    assert any("walked from Python" in str(w.message) and "ma_fft_pow2_c32" in str(w.message) for w in caught)
    assert tb.state == WALK and own.recording is None and not own.bytes and table.cleared == 1
    assert all(getattr(tb, name) is None for name in ("table", "x_in", "a_in", "mask_rows", "att_mask", "pos_all", "g", "out", "dec"))
    assert tb.key == _key() and tb.sightings == 2
    assert own.entry_for(plan, _key(), 7, DIMS, bn) is None and plan.table is tb and tb.state == WALK


def test_over_the_budget_the_first_table_stays_and_the_second_shape_is_walked():
    own, bn = _owner(max_bytes=150), _bn()
    plans, entries = (_ShapePlan(), _ShapePlan()), []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for plan, key in zip(plans, (_key(t2=5), _key(t2=6))):
            own.entry_for(plan, key, 7, DIMS, bn)
            entries.append(own.entry_for(plan, key, 7, DIMS, bn))
            own.recorded(entries[-1])
    first, second = entries
    assert first.state == REPLAY and own.bytes == {first: 100}
    assert second.state == WALK and second.table is None and second.x_in is None
    assert len([w for w in caught if "block_table_max_bytes" in str(w.message)]) == 1
    # (a budget below ONE table still keeps the first: something is always replayed)
    own1, plan1 = _owner(max_bytes=1), _ShapePlan()
    own1.entry_for(plan1, _key(), 7, DIMS, bn)
    tb = own1.entry_for(plan1, _key(), 7, DIMS, bn)
    own1.recorded(tb)
    assert tb.state == REPLAY and own1.bytes == {tb: 100}


def test_a_third_key_on_one_plan_evicts_the_oldest_entry_and_its_ledger_line():
    own, plan, bn = _owner(), _ShapePlan(), _bn()
    entries = []
    for extra in (0, 1):
        own.entry_for(plan, _key(extra=extra), 7, DIMS, bn)
        entries.append(own.entry_for(plan, _key(extra=extra), 7, DIMS, bn))
        own.recorded(entries[-1])
    assert set(own.bytes) == set(entries) and len(plan.tables) == 2
    oldest_table = entries[0].table
    assert own.entry_for(plan, _key(extra=2), 7, DIMS, bn) is None
    assert list(plan.tables) == [_key(extra=1), _key(extra=2)] and set(own.bytes) == {entries[1]}
    assert entries[0].state is None and entries[0].table is None and oldest_table.cleared == 1 and entries[1].state == REPLAY


def test_forgetting_a_plan_and_drop_all_empty_the_ledger():
    own, bn = _owner(), _bn()
    plans = (_ShapePlan(), _ShapePlan(), _ShapePlan())
    entries = []
    for i, plan in enumerate(plans[:2]):
        own.entry_for(plan, _key(t2=5 + i), 7, DIMS, bn)
        entries.append(own.entry_for(plan, _key(t2=5 + i), 7, DIMS, bn))
        own.recorded(entries[-1])
    own.forget_plan(plans[0])  # (what the block-sums cache calls for a plan that leaves it)
    assert own.bytes == {entries[1]: 100} and not plans[0].tables and plans[0].table is None and entries[0].state is None
    own.entry_for(plans[2], _key(t2=9), 7, DIMS, bn)
    rec = own.entry_for(plans[2], _key(t2=9), 7, DIMS, bn)
    assert own.recording is rec
    own.drop_all(plans)
    assert not own.bytes and own.recording is None and all(not p.tables and p.table is None for p in plans)
    assert entries[1].state is None and rec.state is None and rec.table is None
    # ... and every shape starts over: seen, then recorded again
    assert own.entry_for(plans[1], _key(t2=6), 7, DIMS, bn) is None and plans[1].table.state == SEEN


def test_a_shape_walked_after_running_out_of_memory_is_never_offered_a_table_again():
    own, plan, other, bn = _owner(), _ShapePlan(), _ShapePlan(), _bn()
    own.entry_for(other, _key(t2=6), 7, DIMS, bn)
    kept = own.entry_for(other, _key(t2=6), 7, DIMS, bn)
    own.recorded(kept)
    own.entry_for(plan, _key(), 7, DIMS, bn)
    tb = own.entry_for(plan, _key(), 7, DIMS, bn)
    assert own.recording is tb
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        own.out_of_memory((plan, other))
    assert any("out of memory while recording" in str(w.message) for w in caught)
    assert not own.bytes and own.recording is None and not plan.tables and not other.tables and kept.state is None
    assert torch.equal(own.bn_snapshot[0][0], torch.full((4,), 1.0))  # (still there for the caller to put back)
    for extra in (0, 5):  # (whatever the rest of the key says: the shape is what ran out of memory)
        for _ in range(4):
            assert own.entry_for(plan, _key(extra=extra), 7, DIMS, bn) is None and plan.table.state == WALK
    # another shape is recorded as before
    assert own.entry_for(other, _key(t2=6), 7, DIMS, bn) is None
    assert own.entry_for(other, _key(t2=6), 7, DIMS, bn).state == RECORD


def test_a_half_recorded_table_is_replaced_before_it_is_recorded_again():
    own, plan, bn = _owner(), _ShapePlan(), _bn()
    own.entry_for(plan, _key(), 7, DIMS, bn)
    tb = own.entry_for(plan, _key(), 7, DIMS, bn)
    table = tb.table
    tb.restart()
    assert tb.table is table  # (nothing recorded yet)
    table.recorded = 12
    tb.restart()
    assert tb.table is not table and isinstance(tb.table, _Table) and tb.table.recorded == 0 and tb.state == RECORD


# ---- the engine's attributes -------------------------------------------------------------------------------------------------
def test_engine_assigns_every_attribute_in_its_constructor():
    src = open(os.path.join(ROOT, "mindaudio_amd", "train", "engine.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "ConformerCTCTrainStep")

    def assigned(fn):
        out = set()
        for node in ast.walk(fn):
            targets = node.targets if isinstance(node, ast.Assign) else \
                [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
            for t in targets:
                out |= {n.attr for n in ast.walk(t) if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store)
                        and isinstance(n.value, ast.Name) and n.value.id == "self"}
        return out

    methods = {f.name: assigned(f) for f in cls.body if isinstance(f, ast.FunctionDef)}
    born = methods["__init__"] | methods["_build_flat"]
    late = {name: sorted(attrs - born) for name, attrs in methods.items() if attrs - born}
    assert not late, late
    assert len(born) > 60  # (the walk does find the assignments)
    for spelling in ("self.__dict__", "hasattr(self", 'getattr(self, "'):
        assert spelling not in src, spelling
