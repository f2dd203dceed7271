"""Host side of the block launch table (include/mindaudio_amd.h, "a Conformer block's launches from one C call").

`BlockTable.recording()` makes `_lib.load()` hand out a proxy for the duration of one walked step: every replayable C-ABI call made
between `segment(backward, block)` marks is issued as usual AND appended to the table, and every tensor the kernel wrappers allocate
meanwhile is kept referenced by the table (so that the caching allocator can never hand a recorded address to anybody else).  From the
next step of that batch shape on the engine issues each block with one `ma_conformer_block_fwd_train` / `_bwd_train` call.
`TableEntry` is one batch shape's table with its state, `BlockTables` the owner of all entries of an engine.

What is recorded is the reference's training step over the encoder blocks (/root/reference/mindaudio/utils/train_one_step.py:13-48,
models/conformer.py:109-156); the recorder adds no arithmetic of its own."""
import ctypes
import struct
import warnings

from .. import _lib


class _KeepTorch:
    """`torch`, with the allocating calls of the kernel wrappers remembered (train/kernels.py allocates through `_t()`)."""

    def __init__(self, torch, keep):
        self._torch, self._keep = torch, keep

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _held(self, x):
        self._keep.append(x)
        return x

    def empty(self, *a, **k):
        return self._held(self._torch.empty(*a, **k))

    def zeros(self, *a, **k):
        return self._held(self._torch.zeros(*a, **k))

    def empty_like(self, *a, **k):
        return self._held(self._torch.empty_like(*a, **k))

    def zeros_like(self, *a, **k):
        return self._held(self._torch.zeros_like(*a, **k))


class _RecordingLib:
    """The library, with replayable calls copied into the table's current segment."""

    def __init__(self, lib, table):
        self._lib, self._table, self._wrapped = lib, table, {}

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            fn = self._wrapped[name] = self._table._wrap(name, getattr(self._lib, name))
        return fn


def _as_word(argtype, arg):
    if argtype is ctypes.c_void_p:
        if arg is None:
            return 0
        return int(arg.value or 0) if isinstance(arg, ctypes.c_void_p) else int(arg)
    if argtype in (ctypes.c_float, ctypes.c_double):
        return struct.unpack("<q", struct.pack("<d", float(arg)))[0]
    v = int(arg.value) if hasattr(arg, "value") else int(arg)
    return v - (1 << 64) if v >= (1 << 63) else v


class BlockTable:
    def __init__(self):
        self.lib = _lib.load()
        self.handle = ctypes.c_void_p(self.lib.ma_block_table_create())
        if not self.handle:
            raise _lib.MindaudioAmdError("ma_block_table_create failed")
        self.keep = []          # tensors named by the entries (and everything allocated while recording)
        self.where = None       # (backward, block) being recorded
        self.seed = None        # the recorded step's dropout seed: every seed argument must be this (or 0: no dropout)
        self.recorded = 0
        self.broken = None      # why this recording cannot be replayed (the walked step it was taken from is complete all the same)

    def __del__(self):
        try:
            if self.handle:
                self.lib.ma_block_table_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def clear(self):
        """Give up every tensor this table keeps alive (the recorded entries then name freed memory: the table must not be replayed
        again - the engine drops it in the same breath)."""
        del self.keep[:]  # (in place: the allocation proxy holds the same list)
        self.recorded, self.broken = 0, self.broken or "cleared"

    # ---- recording ---------------------------------------------------------------------------------------------------------------
    class _Recording:
        def __init__(self, table, seed):
            self.table, self.seed = table, seed

        def __enter__(self):
            t = self.table
            if _lib.recording() is not None:
                raise _lib.MindaudioAmdError("a block table is already being recorded by this thread")
            t.seed, t.where = int(self.seed), None
            t._proxy = _RecordingLib(t.lib, t)
            _lib.set_recording(t)
            return t

        def __exit__(self, *exc):
            _lib.set_recording(None)
            self.table.where = None
            return False

    def recording(self, seed):
        return BlockTable._Recording(self, seed)

    def segment(self, backward, block):
        """The calls that follow belong to (direction, block); None: not to any block (they are issued but not recorded)."""
        self.where = None if backward is None else (1 if backward else 0, int(block))

    def torch(self, torch):
        kt = self.__dict__.get("_keep_torch")
        if kt is None:
            kt = self._keep_torch = _KeepTorch(torch, self.keep)
        return kt

    def _wrap(self, name, fn):
        proto = _lib.PROTOTYPES.get(name)
        fid = int(self.lib.ma_block_table_entry_point(name.encode())) if proto is not None else -1
        if fid < 0:
            if fid != -2 or name.startswith("ma_block_table_") or name.startswith("ma_conformer_block_"):
                return fn  # size queries, layout helpers, the table's own entry points: nothing to replay

            def refuse(*args):  # issued as usual; the table is marked: the engine keeps walking this batch shape
                if self.where is not None and self.broken is None:
                    self.broken = "%s cannot be replayed from a block table" % name
                return fn(*args)
            return refuse
        argtypes = proto[1]
        seed_mask = int(self.lib.ma_block_table_entry_point_seeds(fid))

        def call(*args):
            rc = fn(*args)
            if self.where is not None and rc == 0 and self.broken is None:
                try:
                    self._add(name, fid, argtypes, seed_mask, args)
                except _lib.MindaudioAmdError as e:  # (the launch itself is done: only the RECORDING failed)
                    self.broken = str(e)
            return rc
        return call

    def _add(self, name, fid, argtypes, seed_mask, args):
        if len(args) != len(argtypes):
            raise _lib.MindaudioAmdError("%s: %d arguments for %d parameters" % (name, len(args), len(argtypes)))
        words, blob = [], bytearray()
        for k, (tp, a) in enumerate(zip(argtypes, args)):
            if isinstance(tp, type) and issubclass(tp, ctypes._Pointer):  # a host struct (or host array of structs)
                if a is None:
                    words.append(-1)
                    continue
                obj = getattr(a, "_obj", None)  # byref(x)
                if obj is None:
                    obj = a.contents if isinstance(a, ctypes._Pointer) else a
                if isinstance(obj, _lib.TrainEpilogue) and obj.seed not in (0, self.seed):
                    raise _lib.MindaudioAmdError("%s: an epilogue with seed %d in a step of seed %d" % (name, obj.seed, self.seed))
                words.append(len(blob))
                raw = bytes(obj)
                blob += raw + b"\0" * (-len(raw) % 8)
                continue
            w = _as_word(tp, a)
            if (seed_mask >> k) & 1 and w not in (0, self.seed):
                raise _lib.MindaudioAmdError("%s: seed argument %d in a step of seed %d" % (name, w, self.seed))
            words.append(w)
        arr = (ctypes.c_int64 * len(words))(*words)
        buf = (ctypes.c_char * len(blob)).from_buffer(blob) if blob else None
        _lib.check(self.lib.ma_block_table_add(self.handle, self.where[0], self.where[1], fid, arr, len(words), buf, len(blob)),
                   "block_table_add(%s)" % name)
        self.recorded += 1

    def nbytes(self):
        """Device bytes this table keeps alive (distinct storages of everything allocated while it was recorded)."""
        seen, total = set(), 0
        for x in self.keep:
            try:
                st = x.untyped_storage()
                key, n = st.data_ptr(), st.nbytes()
            except Exception:
                continue
            if key not in seen:
                seen.add(key)
                total += n
        return total

    # ---- replay ------------------------------------------------------------------------------------------------------------------
    def calls(self, backward, block):
        return int(self.lib.ma_block_table_calls(self.handle, 1 if backward else 0, block))

    def forward(self, block, seed, stream):
        rc = self.lib.ma_conformer_block_fwd_train(self.handle, block, seed, stream)
        if rc != 0:
            _lib.check(rc, "conformer_block_fwd_train(block %d, call %d)" % (block, self.lib.ma_block_table_failed_call(self.handle)))

    def backward(self, block, seed, stream):
        rc = self.lib.ma_conformer_block_bwd_train(self.handle, block, seed, stream)
        if rc != 0:
            _lib.check(rc, "conformer_block_bwd_train(block %d, call %d)" % (block, self.lib.ma_block_table_failed_call(self.handle)))


# ---- the tables of an engine -----------------------------------------------------------------------------------------------------
SEEN, RECORD, REPLAY, WALK = "seen", "record", "replay", "walk"


# One batch shape's launch table: SEEN (walked from Python, counted) -> RECORD (walked AND filled) -> REPLAY (one C call per block), or
# WALK: a shape the table cannot cover or could not be recorded for, walked from Python for good.
class TableEntry:
    """From RECORD on the entry owns the buffers at the blocks' boundary - they live at fixed addresses for as long as the table
    does - and `dec`, the decoder's part of the recording."""

    _BUFFERS = ("table", "x_in", "a_in", "mask_rows", "att_mask", "pos_all", "g", "out", "dec")

    def __init__(self, key):
        self.key, self.state, self.sightings, self.table = key, SEEN, 0, None
        self._release()

    def _release(self):
        if self.table is not None:
            self.table.clear()  # (the recorder's kept tensors: other references to the table must not keep them pinned)
        for name in self._BUFFERS:
            setattr(self, name, None)

    def sighted(self, min_sightings, segments, max_segments):
        """One more step of a SEEN shape: RECORD when this step is the one to record (the caller then calls `record`), WALK when the
        step has more launch segments than a table holds, else SEEN."""
        # (the first step(s) warm the wrappers' pooled buffers and tell a recurring shape from a one-off: a loader that pads to the
        # batch maximum produces many shapes that never come back, and recording each would pin 2-4 GB apiece)
        self.sightings += 1
        if self.sightings < max(2, int(min_sightings)):
            return SEEN
        if segments > int(max_segments):
            self.state = WALK
            return WALK
        return RECORD

    def record(self, table, b, t2, att_shape, d, L, dev):
        import torch

        m, f32, bf = b * t2, dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
        self.state, self.table = RECORD, table
        self.x_in, self.a_in = torch.empty((m, d), **f32), torch.empty((m, d), **bf)
        self.mask_rows, self.att_mask = torch.empty(m, **f32), torch.empty(att_shape, **f32)
        self.pos_all, self.g = torch.empty((t2, L * d), **bf), torch.empty((m, d), **f32)

    def restart(self):  # (a recorded step that raised before its backward pass was complete: start over on an empty table)
        if self.table.recorded:
            self.table = type(self.table)()

    def replay(self):
        self.state = REPLAY

    def walk(self):  # (for good: the table and every buffer go, the key and the count stay)
        self._release()
        self.state = WALK

    def drop(self):  # (the entry leaves its plan: nothing of it may be used again)
        self._release()
        self.state = None


# Every launch table of one engine.  Entries hang on the batch shape's block-sums plan (`plan.tables`, at most two per plan;
# `plan.table`: the one in use) and go with it; this object keeps what spans plans.
class BlockTables:
    """The ledger of device bytes the recorded tables pin and its budget, the entry being recorded (with the BatchNorm running
    statistics of before that step), the shapes walked for good after running out of memory, and the warnings already given."""

    def __init__(self, max_bytes, min_sightings, max_blocks, make_table=BlockTable):
        self.max_bytes, self.min_sightings, self.max_blocks, self._make_table = max_bytes, min_sightings, max_blocks, make_table
        self.bytes, self.warned, self.recording, self.walk_shapes, self.bn_snapshot = {}, set(), None, set(), None

    def warn(self, msg):
        if msg not in self.warned:
            self.warned.add(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=3)

    def entry_for(self, plan, key, segments, dims, bn_stats):
        """The entry to run this step from, None while the shape is walked from Python.  key[:3] = (b, t2, attention-mask shape);
        `dims` = (d, L, device) of the boundary buffers; `bn_stats` = the (mean, var) tensors to snapshot when recording starts."""
        tb = plan.table = plan.tables.get(key)
        if tb is None:
            while len(plan.tables) >= 2:  # (e.g. the padding-mask and the chunk-mask form of one shape)
                self.drop(plan.tables, next(iter(plan.tables)))
            tb = plan.table = plan.tables[key] = TableEntry(key)
        if key[:3] in self.walk_shapes:
            tb.state = WALK
        if tb.state == SEEN:
            state = tb.sighted(self.min_sightings, segments, self.max_blocks)
            if state == WALK:
                self.warn("block tables: %d launch segments > the table's %d: this configuration is walked from Python"
                          % (segments, self.max_blocks))
            if state == RECORD:
                tb.record(self._make_table(), key[0], key[1], key[2], *dims)
                self.recording = tb
                self.bn_snapshot = [(m.clone(), v.clone()) for m, v in bn_stats]
        return tb if tb.state in (RECORD, REPLAY) else None

    def recorded(self, tb):
        """End of a recorded step: the table replays from the next step on - unless the recorder met a call it cannot replay or the
        byte budget of all tables is spent: then THIS shape is walked for good (the tables recorded so far stay)."""
        # (dropping the oldest table instead made a loader's round-robin over its buckets re-record a shape on every step)
        self.recording = None
        if tb.table.broken is not None:
            self.warn("block tables: %s - this batch shape is walked from Python" % tb.table.broken)
            return tb.walk()
        nbytes, pinned = tb.table.nbytes(), sum(self.bytes.values())
        if self.bytes and pinned + nbytes > int(self.max_bytes):
            self.warn("block tables: %.1f GB of launch tables are recorded (block_table_max_bytes); further batch shapes are "
                      "walked from Python" % (pinned / 2 ** 30))
            return tb.walk()
        tb.replay()
        self.bytes[tb] = nbytes

    def drop(self, tables, key):
        tb = tables.pop(key, None)
        if tb is not None:
            self.bytes.pop(tb, None)
            tb.drop()

    def forget_plan(self, plan):  # (it leaves its cache: the ledger must not keep its tables - and their buffers - alive)
        for key in list(plan.tables):
            self.drop(plan.tables, key)
        plan.table = None

    def drop_all(self, plans):
        for plan in plans:
            self.forget_plan(plan)
        self.bytes.clear()
        self.recording = None

    def out_of_memory(self, plans):
        """The recording step ran out of memory: every table goes, its shape is walked for good (the caller restores bn_snapshot)."""
        _lib.set_recording(None)
        self.walk_shapes.add(self.recording.key[:3])
        self.drop_all(plans)
        self.warn("block tables: out of memory while recording a batch shape - tables dropped, the shape is walked from Python")
