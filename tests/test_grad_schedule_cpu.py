"""train/grad_schedule.py on the host alone: which weight-gradient products wait in which group, when a group is launched and which
gradient buckets go on the wire behind it - over walked and replayed steps, the three forms of the block's products, with and without
a decoder, and through steps that stop half way.  The direct groups, the split-K launch, the plan's batched sums and the reducer are
stand-ins that only log; no library, no device."""
from types import SimpleNamespace

import pytest

from mindaudio_amd.train.grad_schedule import GradSchedule

PAIRS = [(12, 6), (12, 5), (2, 6), (7, 3), (1, 1)]   # (encoder blocks, dw_group_blocks)
GRID = PAIRS + [(3, 0), (12, 0)]                      # ... and the split-K arm
MODES = ["direct", "splitk", "noplan"]                # noplan: the one-launch-per-cell path, every sum taken where it is produced
DECODERS = ["none", "plain", "deferred"]
DEC = ("dec.first", "dec.last")


class Group:
    """kernels.DirectGroup: add / launch / clear / n - the launch logs which products left with it."""

    def __init__(self, log):
        self.log, self.items = log, []

    n = property(lambda self: len(self.items))

    def add(self, dy, x, out, colsum):
        self.items.append(out)

    def launch(self):
        if self.items:
            self.log.append(("group",) + tuple(self.items))

    def clear(self):
        self.items = []


def flat(blocks, decoder):
    names = ["conv1_w", "conv1_b", "conv2_w", "conv2_b", "out_w", "out_b", "pos_w"]
    for i in range(blocks):
        names += ["l%d.first" % i, "l%d.mid" % i, "l%d.last" % i]
    names += ["after_norm.g", "after_norm.b", "ctc_w", "ctc_b"]
    if decoder:
        names += ["dec.first", "d0.ca_kv_w", "d0.ff_w1", "dec.last"]
    return SimpleNamespace(index=dict.fromkeys(names), span=lambda ns: (ns[0], ns[-1]))


def make(blocks, group, mode, decoder=True):
    """-> (schedule, its event log, the plan stand-in): built through the constructor, as the engine does."""
    log = []
    owner = SimpleNamespace(reducer=SimpleNamespace(launch=lambda lo, hi: log.append(("bucket", lo, hi))))
    gs = GradSchedule(owner, flat(blocks, decoder), blocks, group, mode == "direct", lambda: Group(log),
                      lambda items, with_colsum: log.append(("splitk",) + tuple(part for _, _, part in items)))
    layers = [SimpleNamespace(reduce=lambda what, li=li: log.append(("block", li))) for li in range(blocks)]
    return gs, log, (None if mode == "noplan" else SimpleNamespace(layers=layers))


ROWS = SimpleNamespace(shape=(40, 256))  # a decoder product's dy: as many rows as the decoder's activations


def step(gs, log, blocks, plan, dec="none", replayed=False, dec_replayed=None, deferred=None, stop=None):
    """One step as the engine drives it (engine._forward_backward); `stop`: the phase at which it raises.  Returns the events of this
    step and what decoder_done returned.  replayed: the encoder's backward runs from its launch table; dec_replayed (default: the
    same): so does the decoder's, with the recorded step's `deferred`."""
    start = len(log)
    dec_replayed = replayed if dec_replayed is None else dec_replayed
    gs.begin_step()
    if dec != "none":
        gs.decoder_begin(40, enc_replayed=replayed)
        log.append(("decoder launches",))
        if dec_replayed:
            deferred = gs.decoder_done(replayed=True, deferred=deferred)
        else:
            if gs.direct:
                gs.queue_decoder(ROWS, None, "d0.ff_w1", None, long_ok=False)
            if stop == "in_decoder":
                return log[start:], None
            if dec == "deferred" and gs.direct and plan is not None:  # (the engine's `merge`: else the product is immediate)
                gs.queue_decoder_long(None, None, "ca_kv", None)
            deferred = gs.decoder_done()
    if stop == "after_decoder":
        return log[start:], deferred
    for li in reversed(range(blocks)):
        log.append(("launches", li))
        if not replayed and plan is not None:
            for k in range(2):
                if gs.direct:
                    gs.queue_block(None, None, ("l", li, k), None)
                else:
                    gs.queue_splitk(None, None, ("l", li, k))
        if stop == "in_block" and li == max(blocks - 2, 0):
            return log[start:], deferred
        gs.block_done(li, plan, replayed=replayed)
    if stop == "before_front":
        return log[start:], deferred
    gs.front_done()
    return log[start:], deferred


def buckets(events):
    return [e[1:] for e in events if e[0] == "bucket"]


def the_table_stands_in_for(e):
    return e[0] in ("block", "group", "splitk")


def cases():
    for dec in DECODERS:
        for replayed in (False, True):
            yield dec, replayed


def run(blocks, group, mode, dec, replayed):
    """-> (the schedule, the events of a walked or replayed step, the walked step it has to match)."""
    gs, log, plan = make(blocks, group, mode, decoder=dec != "none")
    walked, deferred = step(gs, log, blocks, plan, dec)
    assert gs.idle(), (dec, replayed)
    if not replayed:
        return gs, walked, walked
    events, again = step(gs, log, blocks, plan, dec, replayed=True, deferred=deferred)  # (the recorded step's flag, handed back)
    assert gs.idle() and again == deferred, (dec, replayed)
    return gs, events, walked


@pytest.mark.parametrize("dec_pending", [False, True])
@pytest.mark.parametrize("blocks,group", PAIRS)
def test_replayed_backward_launches_the_gradient_buckets_where_the_walked_one_does(blocks, group, dec_pending):
    """N > 1: a finished group's gradient buckets go on the wire (reducer.launch) behind its direct weight-gradient products.  The
    replayed backward pass (one C call per block) must issue the same spans at the same points as the walked one - one function,
    block_done, takes the decisions for both.
    dec_pending (round 6): the decoder's long-contraction weight gradients ride in the encoder's FIRST direct group, so the
    decoder's bucket must leave behind that group - once, in the walked and in the replayed pass alike."""
    logs, scheds = [], []
    for replayed in (False, True):
        gs, log, plan = make(blocks, group, "direct")
        gs.begin_step()
        gs.decoder_begin(40, enc_replayed=replayed)
        if dec_pending:
            gs.queue_decoder_long(None, None, "ca_kv", None)
        for li in reversed(range(blocks)):
            log.append(("launches", li))  # (the table stands in for the block's launches)
            gs.block_done(li, plan, replayed=replayed)
        logs.append(log)
        scheds.append(gs)
    (wlog, rlog), (walked, replayed) = logs, scheds
    assert [e for e in wlog if not the_table_stands_in_for(e)] == rlog
    assert sum(1 for e in rlog if e[0] == "bucket") == blocks + int(dec_pending) and walked.blocks == replayed.blocks == []
    if dec_pending:
        dec = [i for i, e in enumerate(rlog) if e == ("bucket",) + DEC]
        first_group = min(group, blocks)
        launches = [i for i, e in enumerate(rlog) if e[0] == "launches"]
        # exactly once, behind the first group's last block and before the next block's launches
        assert len(dec) == 1 and dec[0] > launches[first_group - 1] and (len(launches) == first_group or dec[0] < launches[first_group])
        assert not walked.dec_deferred and not replayed.dec_deferred
    assert walked.idle() and replayed.idle()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks,group", GRID)
def test_every_bucket_goes_on_the_wire_exactly_once(blocks, group, mode):
    """One step launches the spans of engine.bucket_spans, each once and (pure CTC) in that order; a hybrid step those plus the
    decoder's span, once."""
    from mindaudio_amd.train.engine import bucket_spans

    for dec, replayed in cases():
        gs, events, _ = run(blocks, group, mode, dec, replayed)
        want = bucket_spans(flat(blocks, dec != "none"), blocks)
        assert len(want) == blocks + 2 and want == gs.buckets.ctc_order()
        got = buckets(events)
        if dec == "none":
            assert got == want, (dec, replayed)
        else:
            assert sorted(got) == sorted(want + [DEC]), (dec, replayed)
            assert [s for s in got if s != DEC] == want, (dec, replayed)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks,group", GRID)
def test_no_bucket_leaves_before_the_launch_that_writes_it(blocks, group, mode):
    """A block's bucket never goes before the launch of the group that holds its products (nor before its batched sums); the decoder's
    goes with the end of the decoder's backward - or, deferred, behind the first encoder group and before the next block's launches."""
    for dec, replayed in cases():
        gs, events, _ = run(blocks, group, mode, dec, replayed)
        at = {e: i for i, e in enumerate(events)}
        assert len(at) == len(events)  # (no event twice)
        grouped = gs.direct and mode != "noplan"
        for li in range(blocks):
            bucket = at[("bucket",) + gs.buckets.layers[li]]
            writers = [i for e, i in at.items() if e == ("launches", li) or e == ("block", li)
                       or (e[0] in ("group", "splitk") and ("l", li, 0) in e)]
            assert len(writers) == (1 if replayed or mode == "noplan" else 3), (dec, replayed, li)
            assert bucket > max(writers), (dec, replayed, li)
        launches = [at[("launches", li)] for li in reversed(range(blocks))]
        if dec != "none":
            d = at[("bucket",) + DEC]
            if dec == "deferred" and grouped:
                first = min(group, blocks)
                assert d > launches[first - 1] and (len(launches) == first or d < launches[first]), (dec, replayed)
                if not replayed:
                    assert d > next(i for e, i in at.items() if e[0] == "group" and "ca_kv" in e)
            else:
                assert at[("decoder launches",)] < d < launches[0], (dec, replayed)
            if not replayed and gs.direct:  # the decoder layers' products: one grid before the decoder's bucket
                assert next(i for e, i in at.items() if e[0] == "group" and "d0.ff_w1" in e) < d
        # and the head and the front come last
        assert [at[("bucket",) + s] for s in (gs.buckets.head, gs.buckets.front)] == [len(events) - 2, len(events) - 1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks,group", GRID)
def test_walked_and_replayed_steps_log_the_same_events(blocks, group, mode):
    for dec in DECODERS:
        _, events, walked = run(blocks, group, mode, dec, replayed=True)
        assert not [e for e in events if the_table_stands_in_for(e)]  # a replayed step launches nothing of its own
        assert [e for e in walked if not the_table_stands_in_for(e)] == events, dec


@pytest.mark.parametrize("stop", ["in_decoder", "after_decoder", "in_block", "before_front"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks,group", GRID)
def test_a_step_that_stops_half_way_leaves_no_trace(blocks, group, mode, stop):
    """begin_step is the one reset: after a step that raised inside the decoder, between the decoder's and the encoder's backward,
    inside a block or before the front, it leaves nothing queued and nothing deferred, and the next step logs what a fresh object's
    does."""
    for dec in DECODERS:
        if dec == "none" and stop in ("in_decoder", "after_decoder"):
            continue
        fresh, flog, fplan = make(blocks, group, mode, decoder=dec != "none")
        want, _ = step(fresh, flog, blocks, fplan, dec)
        gs, log, plan = make(blocks, group, mode, decoder=dec != "none")
        step(gs, log, blocks, plan, dec, stop=stop)
        if mode != "noplan" and (stop == "in_block" or (stop == "in_decoder" and gs.direct) or
                                 (stop == "after_decoder" and dec == "deferred" and gs.direct)):
            assert not gs.idle(), (dec, stop)  # (the broken step did leave something: the case is not vacuous)
        gs.begin_step()
        assert gs.idle(), (dec, stop)
        got, _ = step(gs, log, blocks, plan, dec)
        assert got == want and gs.idle(), (dec, stop)


@pytest.mark.parametrize("blocks,group", PAIRS)
def test_replayed_encoder_with_a_walked_decoder_defers_the_bucket_and_queues_nothing(blocks, group):
    """Label widths change from batch to batch (round 6): the decoder is walked from Python while the encoder's backward runs from
    its launch table, whose first recorded group already holds the decoder's long product.  The walk's own copy of that product is
    queued nowhere - nobody would launch it - but the decoder's bucket still waits for that group."""
    gs, log, plan = make(blocks, group, "direct")
    recorded, deferred = step(gs, log, blocks, plan, "deferred")
    assert deferred is True
    events, again = step(gs, log, blocks, plan, "deferred", replayed=True, dec_replayed=False)
    assert again is True and gs.idle() and gs.enc.n == 0
    groups = [e for e in events if e[0] == "group"]
    assert groups == [("group", "d0.ff_w1")]  # the decoder layers' own grid; no encoder group, and "ca_kv" in none
    assert [e for e in recorded if e[0] in ("launches", "decoder launches", "bucket")] == [e for e in events if e[0] != "group"]
