#!/usr/bin/env python3
"""Golden vectors of the CTC prefix beam search and the attention rescoring: the reference's own functions
(mindaudio/utils/recognize.py::ctc_prefix_beam_search, ::attention_rescoring, recognize.py:273-406) run in THIS container behind the
`mindspore` stub of gen_goldens.py.  recognize.Tensor is replaced by an ndarray subclass with asnumpy(), and the models are mocks
whose predict() returns prepared arrays: top-k lists for the CTC side, the log_softmax of float32 decoder logits for the rescoring
side (as float64, so that the reference's score loop sums in float64).  The mock decoder also records the hyps_in_pad /
hyps_sub_masks the reference built.

Writes tests/golden/beam_goldens.npz:
  pb_n                       number of prefix-search cases; per case i (prefix pb{i}_):
  logp (T, beam) f32, index (T, beam) i32, mask (T,) f32  the search's inputs
  hyp (beam, T) i32, len (beam,) i32, score (beam,) f64, n () i32   the reference's hypotheses (best first), zero padded
  rs_n                       number of rescoring cases; per case i (prefix rs{i}_): the prefix-search inputs and outputs as above, plus
  logits (beam, 31, V) f32, eos, sos, ctc_weight, best (chosen slot), best_score f64, hyps_in_pad (beam, 31) i32,
  hyps_sub_masks (beam, 31, 31) f32

usage: python tests/golden/gen_beam_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_goldens import _load, load_reference  # noqa: E402


class _Tensor(np.ndarray):
    def __new__(cls, x, dtype=None):
        return np.asarray(x).view(cls)

    def asnumpy(self):
        return np.asarray(self)


def _topk(rng, T, V, k, kind):
    """float32 log_softmax of random logits, the k best per frame (descending, lower index first on ties)."""
    if kind == "peaky":
        x = rng.randn(T, V).astype(np.float32)
        hot = rng.randint(0, V, size=T)
        hot[rng.rand(T) < 0.5] = 0  # blank-dominated frames, as a trained CTC head gives
        x[np.arange(T), hot] += 8.0
    elif kind == "flat":
        x = (0.1 * rng.randn(T, V)).astype(np.float32)
    elif kind == "ninf":  # -inf logits (a vocabulary mask): -inf log-probabilities in the top-k lists, -inf candidates in the beam
        x = np.full((T, V), -np.inf, np.float32)
        x[:, 0] = np.where(rng.rand(T) < 0.5, rng.randn(T), -np.inf)
        x[np.arange(T), rng.randint(0, V, size=T)] = 0.5
    else:
        x = rng.randn(T, V).astype(np.float32)
    m = x.max(1, keepdims=True)
    lp = ((x - m) - np.log(np.exp(x - m).sum(1, keepdims=True))).astype(np.float32)
    order = np.stack([np.lexsort((np.arange(V), -lp[t]))[:k] for t in range(T)])
    return np.take_along_axis(lp, order, 1).astype(np.float32), order.astype(np.int32)


class _CtcModel:
    def __init__(self, logp, index, mask):
        self.out = (_Tensor(np.zeros((1, logp.shape[0], 4), np.float32)), _Tensor(mask.astype(np.float32)), _Tensor(logp),
                    _Tensor(index))

    def predict(self, *a):
        return self.out


class _RescoreModel:
    def __init__(self, logits):
        self.logits = logits
        self.seen = None

    def predict(self, encoder_out, encoder_mask, hyps_in_pad, hyps_sub_masks):
        self.seen = (np.asarray(hyps_in_pad).copy(), np.asarray(hyps_sub_masks).copy())
        x = self.logits.astype(np.float64)
        m = x.max(-1, keepdims=True)
        return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _pack(hyps, beam, T):
    hyp = np.zeros((beam, T), np.int32)
    lens = np.zeros(beam, np.int32)
    score = np.full(beam, -np.inf)
    for p, (pre, sc) in enumerate(hyps):
        hyp[p, :len(pre)] = pre
        lens[p] = len(pre)
        score[p] = sc
    return hyp, lens, score


def main():
    load_reference()
    rec = _load("mindaudio.utils.recognize", "mindaudio/utils/recognize.py")
    rec.Tensor = _Tensor
    rng = np.random.RandomState(20261016)
    out = {}
    cases = []
    # (beam, T, V, kind, mask kind)
    for beam in (1, 4, 10, 16):
        cases += [(beam, 40, 6 if beam < 6 else beam + 1, "random", "full"),       # small V: repeats, merges, -inf candidates
                  (beam, 57, 4233, "peaky", "tail"),
                  (beam, 33, 30, "flat", "holes"),
                  (beam, 25, max(beam, 12), "random", "holes")]
    cases += [(10, 249, 4233, "peaky", "tail"), (4, 20, 9, "random", "one"), (10, 12, 11, "random", "none"),
              (16, 16, 16, "random", "full"), (16, 6, 16, "flat", "full"), (10, 3, 10, "random", "full"),
              (4, 14, 6, "ninf", "full"), (10, 18, 12, "ninf", "holes"), (10, 2, 12, "ninf", "full"),
              (16, 3, 20, "ninf", "full")]
    for n, (beam, T, V, kind, mk) in enumerate(cases):
        logp, index = _topk(rng, T, V, beam, kind)
        mask = np.ones(T, np.float32)
        if mk == "tail":
            mask[T - T // 4:] = 0
        elif mk == "holes":
            mask[rng.rand(T) < 0.25] = 0
        elif mk == "one":
            mask[:] = 0
            mask[T // 2] = 1
        elif mk == "none":
            mask[:] = 0
        hyps, _, _ = rec.ctc_prefix_beam_search(_CtcModel(logp, index, mask), np.zeros((1, 4 * T + 8, 2)),
                                                np.ones((1, 1, 4 * T + 8)), beam, None)
        hyp, lens, score = _pack(hyps, beam, T)
        p = "pb%d_" % n
        out.update({p + "logp": logp, p + "index": index, p + "mask": mask, p + "hyp": hyp, p + "len": lens, p + "score": score,
                    p + "n": np.int32(len(hyps))})
    out["pb_n"] = np.int32(len(cases))
    # rescoring: (beam, T, V, kind, ctc_weight)
    rs = [(4, 20, 14, "random", 0.0), (10, 28, 23, "peaky", 0.3), (10, 30, 17, "random", 0.5), (4, 12, 9, "flat", 0.3),
          (10, 24, 40, "random", 0.0), (16, 26, 20, "random", 0.5)]
    for n, (beam, T, V, kind, w) in enumerate(rs):
        logp, index = _topk(rng, T, V, beam, kind)
        mask = np.ones(T, np.float32)
        mask[T - 2:] = 0
        logits = (2.0 * rng.randn(beam, 31, V)).astype(np.float32)
        eos = sos = V - 1
        dec = _RescoreModel(logits)
        ctc = _CtcModel(logp, index, mask)
        hyps, _, _ = rec.ctc_prefix_beam_search(ctc, np.zeros((1, 4 * T + 8, 2)), np.ones((1, 1, 4 * T + 8)), beam, None)
        best, best_score = rec.attention_rescoring(ctc, dec, np.zeros((1, 4 * T + 8, 2)), np.ones((1, 1, 4 * T + 8)), None, sos, eos,
                                                   beam, w)
        slot = [h[0] for h in hyps].index(tuple(best))
        hyp, lens, score = _pack(hyps, beam, T)
        p = "rs%d_" % n
        out.update({p + "logp": logp, p + "index": index, p + "mask": mask, p + "hyp": hyp, p + "len": lens, p + "score": score,
                    p + "n": np.int32(len(hyps)), p + "logits": logits, p + "eos": np.int32(eos), p + "sos": np.int32(sos),
                    p + "ctc_weight": np.float64(w), p + "best": np.int32(slot), p + "best_score": np.float64(best_score),
                    p + "hyps_in_pad": dec.seen[0].astype(np.int32), p + "hyps_sub_masks": dec.seen[1].astype(np.float32)})
    out["rs_n"] = np.int32(len(rs))
    path = os.path.join(HERE, "beam_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
