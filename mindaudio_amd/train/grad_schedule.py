"""Who waits where during the backward pass of the training step (train/engine.py): which weight-gradient products wait in which
group, when a group is launched, and which slice of the flat gradient goes to the all-reduce behind it."""
# ONE owner for the queues, the deferred decoder bucket and the bucket tables; walked and replayed steps take the same decisions here.
# Nothing in this module touches the device but through the two kernel-side objects it is given (a direct group, the split-K grouped
# launch), the plan's batched sum and `owner.reducer.launch` - so the state machine runs on the CPU with stand-ins
# (tests/test_grad_schedule_cpu.py).


def half_of(li):
    """The half of a block-sums plan's arena that block li's partials use: block li + 2 used it last, block li - 1 never does."""
    return li & 1


class Buckets:
    """(lo, hi) of every gradient bucket of the flat layout `fp`: blocks 0 .. L-1, head, front, decoder (None: no decoder)."""

    def __init__(self, fp, L):
        self.layers = [fp.span([n for n in fp.index if n.startswith("l%d." % i)]) for i in range(L)]
        self.head = fp.span(["after_norm.g", "ctc_b"])
        self.front = fp.span(["conv1_w", "conv1_b", "conv2_w", "conv2_b", "out_w", "out_b", "pos_w"])
        dec = [n for n in fp.index if n.startswith("dec.") or (n[0] == "d" and n[1].isdigit())]
        self.dec = fp.span(dec) if dec else None

    def ctc_order(self):
        """The buckets of a pure CTC step in launch order: blocks L-1 .. 0, then the head and the front."""
        return self.layers[::-1] + [self.head, self.front]


# `owner.reducer.launch(lo, hi)` (looked up at every call) takes every bucket.  group_blocks = G and `direct`: a block's direct products
# wait for those of the next G - 1 blocks and leave as one grid, the G buckets behind it; otherwise a block's split-K products leave as
# one grouped launch when the block is done, its bucket behind them.  `direct_group()` -> an object with add(dy, x, out, colsum) /
# launch() / clear() / n (kernels.DirectGroup), `splitk_launch(items, with_colsum=True)` (kernels.gemm_tn_partial_group).
class GradSchedule:
    """A step: begin_step, [decoder_begin, queue_decoder* / queue_decoder_long, decoder_done], per block L-1 .. 0 [queue_block* |
    queue_splitk*, block_done], front_done - after which idle() holds."""

    def __init__(self, owner, fp, L, group_blocks, direct, direct_group, splitk_launch):
        self.owner, self.buckets, self._splitk_launch = owner, Buckets(fp, L), splitk_launch
        self.group_blocks, self.direct = int(group_blocks), bool(direct) and int(group_blocks) > 0
        # splitk: (dy, x, arena slice) of the current block; enc / dec: the direct groups of the encoder blocks and of the decoder's
        # layers; blocks: finished blocks whose buckets wait for the current group
        self.splitk, self.blocks = [], []
        self.enc, self.dec = (direct_group(), direct_group()) if self.direct else (None, None)
        self.begin_step()

    def begin_step(self):
        """The one reset: a step that raised mid-backward must not leave stale products, pinned operands or a deferred bucket behind."""
        self.splitk.clear()
        self.blocks.clear()
        if self.direct:
            self.enc.clear()
            self.dec.clear()
        # dec_deferred: some decoder weight gradients ride in the encoder's first group, so the decoder's bucket leaves behind it
        # enc_replayed: the ENCODER's backward runs from its launch table in this step (its first group holds the decoder's long product)
        # dec_rows: rows of the decoder's activations (what a decoder product's contraction length is compared with)
        self.dec_deferred, self.enc_replayed, self.dec_rows = False, False, 1

    def idle(self):
        """Nothing queued, nothing deferred (a few attribute reads: the engine asserts it at the end of every step)."""
        return not (self.splitk or self.blocks or self.dec_deferred or (self.direct and (self.enc.n or self.dec.n)))

    def _bucket(self, span):
        if span is not None:
            self.owner.reducer.launch(*span)

    # ---- where a product waits ------------------------------------------------------------------------------------------------------
    def queue_block(self, dy, x, out, colsum):
        """A direct product of the current encoder block: issued with its group (block_done)."""
        self.enc.add(dy, x, out, colsum)

    def queue_splitk(self, dy, x, part):
        """A split-K product of the current encoder block, partials into `part`: the block's products leave as ONE grouped launch."""
        self.splitk.append((dy, x, part))

    def decoder_begin(self, rows, enc_replayed):
        self.dec_rows, self.enc_replayed = rows, bool(enc_replayed)

    # A decoder layer's direct product: with the others of the decoder in ONE grid at the end of its backward pass (they were 43 split-K
    # products + 88 reduction launches of ~10 us each: the hybrid step's decoder is launch-bound).
    # long_ok: a product over the ENCODER's rows (ca_kv_w: dkv^T memory, 10 200 rows against the decoder's 1 240) may join the encoder's
    # first group instead - in the decoder's grid its 2 tiles per layer ran 400 us with 244 CUs idle behind them (the grid lasts as long
    # as its longest tile); 234 + 12 tiles are still one resident round, every tile with a full-length contraction.  (The caller allows
    # it only with the launch tables off: a replayed encoder group holds the operands of the step it was recorded in - the fused decoder
    # walk keeps its one long operand at a fixed address for that, the per-layer form does not.)
    def queue_decoder(self, dy, x, out, colsum, long_ok):
        if long_ok and dy.shape[0] > 4 * self.dec_rows:
            self.queue_decoder_long(dy, x, out, colsum)
        else:
            self.dec.add(dy, x, out, colsum)

    # A replayed encoder backward has the item in its recorded group - same operands, same addresses: queueing it here as well would
    # leave it in a group nobody launches, with operands that die with this step.  The bucket is deferred all the same.
    def queue_decoder_long(self, dy, x, out, colsum):
        """A decoder product that rides in the encoder's first group; the decoder's bucket goes on the wire behind that group."""
        if not self.enc_replayed:
            self.enc.add(dy, x, out, colsum)
        self.dec_deferred = True

    # ---- when a group leaves, and the buckets behind it -----------------------------------------------------------------------------
    def decoder_done(self, replayed=False, deferred=None):
        """The decoder's backward is complete: its layers' products as one grid, then its bucket unless that is deferred.  Returns
        whether it is: a recorded step keeps that and hands it back as `deferred` when it is replayed (the table issues the grid)."""
        if replayed:
            self.dec_deferred = bool(deferred)
        elif self.direct:
            self.dec.launch()
            self.dec.clear()
        if not self.dec_deferred:
            self._bucket(self.buckets.dec)
        return self.dec_deferred

    def block_done(self, li, plan, replayed=False):
        """Backward of block li is complete (plan: the shape's block-sums plan, None = every sum was taken where it was produced).
        replayed: the launch table has issued what is launched here; the bucket decisions are the same."""
        if not replayed:
            if self.splitk:
                self._splitk_launch(self.splitk, with_colsum=True)  # the block's eight products: one grid
                self.splitk.clear()
            if plan is not None:
                # the block's partial sums (split-K products, LayerNorm, depthwise convolution, attention biases): one launch
                plan.layers[li].reduce("reduce_splits_batch")
        self.blocks.append(li)
        if not (self.direct and plan is not None) or len(self.blocks) >= self.group_blocks or li == 0:
            # the group's direct products as one grid, its gradient buckets behind it - they can go on the wire while earlier blocks
            # are still being differentiated - then the deferred decoder bucket
            if self.direct and not replayed:
                self.enc.launch()
                self.enc.clear()
            for b in self.blocks:
                self._bucket(self.buckets.layers[b])
            self.blocks.clear()
            if self.dec_deferred:
                self.dec_deferred = False
                self._bucket(self.buckets.dec)

    def front_done(self):
        self._bucket(self.buckets.head)
        self._bucket(self.buckets.front)
