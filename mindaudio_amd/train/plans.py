"""Per-shape plans of the training step (train/engine.py): the item tables of its batched launches, the cache that keeps one plan per
batch shape on a grow-only arena, and the three kinds of plan kept that way.  Nothing here launches but `ItemTable.reduce`."""
import ctypes

import numpy as np
import torch

from .. import _host, _lib
from .grad_schedule import half_of


# The device side of one batched launch (ma_transpose_batch_bf16, ma_pack_batch_bf16, ma_reduce_splits_batch_f32): the packed item
# structs, the workgroup -> item map and the grid size.  Building one costs TWO synchronous host-to-device copies (items, map) - the
# host's whole lead over the device - which is why every user builds its table once per shape and keeps it.
class ItemTable:
    """`entries`: (ctypes struct, number of workgroups) in launch order; each item's `first_block` is filled in here."""

    def __init__(self, entries, device):
        entries = list(entries)
        block_item, first = [], 0
        for i, (item, nblk) in enumerate(entries):
            item.first_block = first
            block_item += [i] * nblk
            first += nblk
        raw = (type(entries[0][0]) * len(entries))(*(item for item, _ in entries))
        self.items = torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).to(device)
        self.block_item = torch.tensor(block_item, dtype=torch.int32, device=device)
        self.n_blocks = first
        self.args = (self.items.data_ptr(), self.block_item.data_ptr(), first)  # (items_ptr, map_ptr, n_blocks) of the C call

    def reduce(self, what):  # (a table of ReduceItems: the batched sum on the current stream)
        _lib.check(_lib.load().ma_reduce_splits_batch_f32(*self.args, _host.current_stream_ptr()), what)


# key -> plan of the last `bound` batch shapes (most recently used last), all on ONE grow-only arena.  ONE rule for growth: the plans
# built on the previous arena name its addresses, so they all go.
class PlanCache:
    """`grow(need, old)` -> elements of the new arena; `on_drop(plan)` sees every plan that leaves, by growth or as the oldest."""

    def __init__(self, bound, grow, dtype, device, on_drop=lambda plan: None):
        self.plans, self.arena, self.bound = {}, None, bound
        self._grow, self._dtype, self._device, self._on_drop = grow, dtype, device, on_drop

    def get(self, key):
        plan = self.plans.pop(key, None)
        if plan is not None:
            self.plans[key] = plan
        return plan

    def arena_for(self, need):  # (the arena, at least `need` elements long)
        old = self.arena.numel() if self.arena is not None else 0
        if self.arena is None or old < need:
            self.arena = torch.empty(self._grow(need, old), dtype=self._dtype, device=self._device)
            while self.plans:
                self._drop(next(iter(self.plans)))
        return self.arena

    def put(self, key, plan):
        self.plans[key] = plan
        while len(self.plans) > self.bound:
            self._drop(next(iter(self.plans)))
        return plan

    def _drop(self, key):
        self._on_drop(self.plans.pop(key))


# (ReduceItem, workgroups): 16 outputs per workgroup for a "tall" item (many partials per output), else 1024
def _reduce_item(part, out, mn, ldo, n_cols, splits, pstride, tall, accumulate=True):
    item = _lib.ReduceItem(part, out.data_ptr(), mn, ldo, n_cols, splits, 1.0, (1 if accumulate else 0) | (2 if tall else 0), 0, pstride)
    return item, (mn + 15) // 16 if tall else (mn + 1023) // 1024


# ---- a block's deferred parameter-gradient sums -----------------------------------------------------------------------------------
DW_SUFFIXES = ("ffm_w1", "ffm_w2", "qkv_w", "o_w", "pw1_w", "pw2_w", "ff_w1", "ff_w2")
LN_SITES = ("norm_final", "norm_ff", "norm_conv", "norm_mha", "norm_ff_macaron")


# off[site] = (offset, bytes, splits) inside one half of the arena (alternate blocks use alternate halves); layers[li] = block li's
# ItemTable; tables / table: the launch-table entries recorded on this plan and the one in use (block_table.BlockTables); dkv_all: the
# decoder's memory-side gradient operand, at one address for the life of the plan
class BlockSumsPlan:
    def __init__(self, m, t2, arena, off, layers, half):
        self.m, self.t2, self.arena, self.off, self.layers, self.half = m, t2, arena, off, layers, half
        self.att_ws = self.dpos_all = self.dkv_all = self.table = None
        self.tables = {}


# Deferred parameter-gradient sums of a block (bf16 mode): the eight weight-gradient products write their split-K partials (and one
# partial bias-gradient vector per split) and the five LayerNorm backward launches their per-workgroup (dgamma | dbeta) partials into
# ONE arena that all blocks share, and ONE launch per block adds them into the flat gradient in a fixed order
# (ma_reduce_splits_batch_f32) instead of a 6 us reduction launch per product / per LayerNorm.
def block_sums_plan(cache, m, t2, fp, dev, L, d, heads, ks, fused, ln_bwd_fused, ffn_bwd_one_launch, chain_final, direct):
    """`direct`: the weight-gradient products write the flat gradient themselves; `chain_final`: norm_final's backward runs in the
    block above's macaron launch."""
    lib = _lib.load()
    off, total = {}, 0
    for sfx in () if direct else DW_SUFFIXES:
        mo, no = fp.w("l0." + sfx).shape
        nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, m))
        off[sfx] = (total, nbytes, int(lib.ma_gemm_tn_splits(mo, no, m)))
        total += (nbytes + 255) // 256 * 256
    ln_parts = int(lib.ma_layernorm_bwd_parts(m))
    fused_parts = int(lib.ma_gemm_rows_train_parts(m))  # sites whose backward rides on an input-gradient product (ln_bwd_fused)
    ffn_parts = int(lib.ma_ffn_train_parts(m))          # ... or on the feed-forward module's one-launch backward
    most = max(ln_parts, fused_parts, ffn_parts)
    for site in LN_SITES:
        # (the region keeps the largest size; the item's split count is what the site's producer really writes)
        parts = fused_parts if (fused and ln_bwd_fused and site != "norm_final") else ln_parts
        if ffn_bwd_one_launch and site in ("norm_ff", "norm_ff_macaron"):
            parts = ffn_parts
        off[site] = (total, most * 512 * 4, parts)
        total += most * 512 * 4
    # the depthwise convolution's per-workgroup (d_dw_w | d_dw_b) partials (fused path)
    cm_parts = int(lib.ma_convmid_bwd_parts(m // t2, t2))
    cm_width = d * (ks + 1)
    off["convmid"] = (total, cm_parts * cm_width * 4, cm_parts)
    total += (cm_parts * cm_width * 4 + 255) // 256 * 256
    # the attention backward's workspace (its dpos / du / dv partials are reduced by the block's launch too) and the buffer the
    # positional projections' gradients of all blocks accumulate in
    b_att = m // t2
    att_bytes = int(lib.ma_relpos_attention_bwd_workspace_bytes(b_att, t2, heads, d // heads))
    dp_off, bias_off, tp_, pph = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(lib.ma_relpos_attention_bwd_layout(b_att, t2, heads, d // heads, ctypes.byref(dp_off),
                                                  ctypes.byref(bias_off), ctypes.byref(tp_), ctypes.byref(pph)), "attention layout")
    total = (total + 255) // 256 * 256
    off["att_ws"] = (total, att_bytes, 0)
    total += (att_bytes + 255) // 256 * 256
    off["dpos_all"] = (total, t2 * L * d * 4, 0)
    total += (t2 * L * d * 4 + 255) // 256 * 256
    # Two copies of the arena, used by alternate blocks (grad_schedule.half_of): block li's partials and block li - 1's never share bytes.
    # (Needed when the sums ran on a second stream; kept on the one stream so that every launch keeps its addresses.)
    half = (total + 255) // 256 * 256
    arena = cache.arena_for(2 * half)
    layers = []
    for li in range(L):
        items, base = [], arena.data_ptr() + half_of(li) * half
        add = lambda *a, **kw: items.append(_reduce_item(*a, **kw))  # noqa: E731
        for sfx in () if direct else DW_SUFFIXES:
            g = fp.g("l%d.%s" % (li, sfx))
            gb = fp.g("l%d.%s" % (li, sfx.replace("_w", "_b")))
            mo, no = g.shape
            o, nbytes, splits = off[sfx]
            add(base + o, g, mo * no, g.stride(0), no, splits, 0, False)
            add(base + o + splits * mo * no * 4, gb, mo, mo, mo, splits, 0, False)   # bias: partial column sums
        for site in LN_SITES:
            o, nbytes, parts = off[site]
            if site == "norm_final" and chain_final and li < L - 1:
                parts = ffn_parts  # written by block li + 1's macaron backward launch (ln_final_chained)
            gg = fp.g("l%d.%s.g" % (li, site))  # (g | b): 2 x 256 contiguous floats of the flat gradient
            assert fp.index["l%d.%s.b" % (li, site)][0] == fp.index["l%d.%s.g" % (li, site)][0] + 256
            add(base + o, gg, 512, 512, 512, parts, 512, True)
        if fused:
            o, nbytes, parts = off["convmid"]
            add(base + o, fp.g("l%d.dw_w" % li), d * ks, d * ks, d * ks, parts, cm_width, True)
            add(base + o + d * ks * 4, fp.g("l%d.dw_b" % li), d, d, d, parts, cm_width, True)
            dk = d // heads
            ws_ptr = base + off["att_ws"][0]
            dpos_l = arena[off["dpos_all"][0]:off["dpos_all"][0] + off["dpos_all"][1]].view(torch.float32).view(t2, L * d)
            # dpos[t][c] of block li += sum over the batch of dp_part[b][t][c]
            # (stored, not accumulated: every block writes its own 256 columns once per step, so dpos_all needs no zero fill)
            # ("tall": one partial per utterance in flight per thread group - as a short item, 64 workgroups walked the 40
            # partials in five dependent rounds of HBM latency, the longest chain of the block's batched sum)
            add(ws_ptr + dp_off.value * 4, dpos_l[:, li * d:(li + 1) * d], t2 * d, L * d, d, b_att, tp_.value * d, True,
                accumulate=False)
            for h in range(heads):  # du[h], dv[h] += sum over the (utterance, query block) partials of head h
                hb = ws_ptr + (bias_off.value + h * pph.value * 128) * 4
                add(hb, fp.g("l%d.u" % li)[h], dk, dk, dk, pph.value, 128, True)
                add(hb + dk * 4, fp.g("l%d.v" % li)[h], dk, dk, dk, pph.value, 128, True)
        layers.append(ItemTable(items, dev))
    plan = cache.put((m, t2), BlockSumsPlan(m, t2, arena, off, layers, half))
    if fused:
        o, nb, _ = off["att_ws"]
        plan.att_ws = (arena[o:o + nb], arena[half + o:half + o + nb])
        o, nb, _ = off["dpos_all"]
        plan.dpos_all = arena[o:o + nb].view(torch.float32).view(t2, L * d)
    return plan


# ---- the three weight gradients outside the blocks --------------------------------------------------------------------------------
class SumsPlan:
    """Partials in `arena` (at off[name] = (offset, bytes, splits), or the views bufs[site]) and the ItemTable that adds them up."""

    def __init__(self, arena, sums, off=None, bufs=None):
        self.arena, self.sums, self.off, self.bufs = arena, sums, off, bufs


# The three weight gradients outside the blocks (CTC head, embed layer, positional projections): split-K partials into one arena, one
# batched sum at the end of the backward pass instead of five reduction launches (fused bf16 path).
def front_plan(cache, m, t2, fp, dev, L, d, f2, V, Vp):
    lib = _lib.load()
    prods = (("ctc", Vp, d, m, V, fp.g("ctc_w"), fp.g("ctc_b")),
             ("out", d, f2 * d, m, d, fp.g("out_w"), fp.g("out_b")),
             ("pos", L * d, d, t2, L * d, fp.g("pos_w"), None))
    off, total = {}, 0
    for name, mo, no, kc, mo_store, _, _ in prods:
        nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, kc))
        off[name] = (total, nbytes, int(lib.ma_gemm_tn_splits(mo, no, kc)))
        total += (nbytes + 255) // 256 * 256
    arena = cache.arena_for(total)
    items = []
    for name, mo, no, kc, mo_store, gw, gb in prods:
        o, _, splits = off[name]
        items.append(_reduce_item(arena.data_ptr() + o, gw, mo_store * no, gw.stride(0), no, splits, 0, False))
        if gb is not None:
            items.append(_reduce_item(arena.data_ptr() + o + splits * mo_store * no * 4, gb, mo_store, mo_store, mo_store, splits, 0,
                                      False))
    return cache.put((m, t2), SumsPlan(arena, ItemTable(items, dev), off=off))


# ---- the decoder's LayerNorm partials ---------------------------------------------------------------------------------------------
# The decoder's 3 Ld + 1 LayerNorm backwards leave their per-workgroup (dgamma | dbeta) partials in one arena and ONE batched launch
# adds them into the flat gradient at the end of the decoder's backward pass (19 reduction launches of 5.6 us fewer per hybrid step;
# the encoder blocks do the same per block).  One plan per row count md = B x (longest label + 1), which changes from batch to batch on
# real data; a launch table that recorded a plan keeps it - and through it the arena - alive itself.
def dec_ln_plan(cache, md, fp, dev, Ld):
    parts = int(_lib.load().ma_layernorm_bwd_parts(md))
    sites = ["dec.after_norm"] + ["d%d.%s" % (li, ln) for li in range(Ld) for ln in ("norm1", "norm2", "norm3")]
    arena = cache.arena_for(len(sites) * parts * 512)
    items, bufs = [], {}
    for i, site in enumerate(sites):
        gg = fp.g(site + ".g")  # (g | b): 2 x 256 contiguous floats of the flat gradient
        assert fp.index[site + ".b"][0] == fp.index[site + ".g"][0] + 256
        bufs[site] = arena[i * parts * 512:(i + 1) * parts * 512]
        items.append(_reduce_item(bufs[site].data_ptr(), gg, 512, 512, 512, parts, 512, True))
    return cache.put(md, SumsPlan(arena, ItemTable(items, dev), bufs=bufs))
