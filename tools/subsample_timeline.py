"""Phase timeline of subsample_fused_kernel from a -DMA_SF_PROF build of subsample_fused.hip
(SRC=subsample_fused.hip bash tools/ffn_variants.sh build "prof:-DMA_SF_PROF"; run with MINDAUDIO_AMD_LIB=.../variants/prof.so;
MINDAUDIO_AMD_SUBSAMPLE=tile times the one-tile-per-workgroup kernel instead of the walking one):
s_memtime stamps of consumer wave 0 and producer wave 4 of three workgroups (the first, the middle one, the sixth from the end of
the grid) for four tiles of each workgroup's walk - its first, the middle one, the one after that, its last - in shader-clock
cycles since the workgroup's entry.  The one-tile kernel has one tile per workgroup: only "first" is printed."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mindaudio_amd import _lib, ops

lib = _lib.load()
B, T, F = 64, 1000, 80
feats = torch.randn(B, F, T + 1, device="cuda").transpose(1, 2)[:, :T]
w1 = (torch.randn(256, 9, device="cuda") * 0.3).contiguous()
b1 = torch.randn(256, device="cuda") * 0.1
w2 = (torch.randn(256, 3, 3, 256, device="cuda") / 48).bfloat16()
b2 = torch.randn(256, device="cuda")
spk = ops.subsample_fused_pack(w1, w2, F)
fn = lambda: ops.subsample_fused(feats, spk, b1, b2)
for _ in range(5):
    fn()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    fn()
e1.record()
torch.cuda.synchronize()
print("launch %.1f us (back to back, instrumented build)" % (e0.elapsed_time(e1) / 20 * 1e3))
lib.ma_debug_sf_prof.argtypes = [ctypes.c_void_p]
acc = []
for it in range(10):
    fn()
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * 768)()
    assert lib.ma_debug_sf_prof(buf) == 0
    a = np.array(buf[:], dtype=np.int64).reshape(2, 3, 4, 32)
    # cycles since the workgroup's entry (consumer wave 0's first stamp); stamps that were never written stay 0
    acc.append(np.where(a != 0, a - a[0, :, 0, 0][None, :, None, None], 0))
a = np.median(np.stack(acc), axis=0)
TILES = ("first", "middle", "middle + 1", "last")
for role, name in ((0, "consumer wave 0"), (1, "producer wave 4")):
    labels = {0: "entry / join barrier passed", 1: "rows staged", 2: "X built", 3: "patch 0 built",
              20: "B7 passed" if role else "Bx passed (chunk 7 left by all)", 21: "epilogue end",
              22: "next rows requested", 23: "next rows written", 24: "next X built", 27: "Bx passed", 25: "next patch 0 built"}
    for k in range(8):
        labels[4 + 2 * k] = ("chunk %d start" % k) if role == 0 else ("patch %d start" % (k + 1))
        labels[5 + 2 * k] = ("chunk %d end" % k) if role == 0 else ("patch %d built" % (k + 1))
    order = sorted(labels, key=lambda k: {22: 16.3, 17: 16.6, 23: 17.5, 20: 18, 24: 24, 27: 24.5, 25: 25}.get(k, k) if role else k)
    for ts, tname in enumerate(TILES):
        if not a[role, :, ts, :].any():
            continue
        print("== %s, the workgroup's %s tile: cycles since the workgroup's entry, three workgroups" % (name, tname))
        prev = None
        for k in order:
            v = a[role, :, ts, k]
            if not v.any() and not (k == 0 and ts == 0 and role == 0):
                continue
            d = "" if prev is None else "  (+%s)" % " / ".join("%6d" % int(x) for x in (v - prev))
            print("%-32s %s%s" % (labels[k], " / ".join("%8d" % int(x) for x in v), d))
            prev = v
if a[0, :, 2, 4].any():
    gap = a[0, :, 2, 4] - a[0, :, 1, 19]
    print("consumer wave 0, end of chunk 7 of the middle tile -> start of chunk 0 of the next: %s cycles"
          % " / ".join("%d" % int(x) for x in gap))
