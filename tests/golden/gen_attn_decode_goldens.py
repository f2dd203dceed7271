#!/usr/bin/env python3
"""Golden vectors of the autoregressive `attention` decode mode: the reference's own recognize() (mindaudio/utils/recognize.py:78-251)
in its full_graph=False NumPy form, run behind the `mindspore` stub of gen_goldens.py.  recognize.Tensor is
replaced by an ndarray subclass with asnumpy() (and a view() that reshapes, as mindspore's does).  The model is a mock:
  predict_network.backbone.acc_net.encoder  returns a prepared (1, maxlen, 4) array and its mask
  predict_network.add_flags_recursive       does nothing
  predict()                                 states PredictNet.construct (models/decoders/decoder_factory.py:372-413) in float32 NumPy
                                            with the reference's own mask_finished_scores, mask_finished_preds and topk_fun
The decoder's logits are a deterministic float32 function of the row's prefix, built from tables: a score g(prefix, v) = bigram table
[last token, v] + half a second table [token before, v] + a positional table [position, v], plus an eos bias that grows with the
position (so that beams finish at different steps); the best token of a row gets the logit 0 and every other token -(30 + its
distance to the best).  All values are multiples of 1/8 (1 in the `ties` case), hence exact in float32, and with every other logit
at or below -30 the float32 sum of exponentials rounds to 1: log_softmax is the identity whatever exp / log an implementation uses.
So a search that takes its log-probabilities from these logits can be compared with the reference bit for bit, scores included, and
exact ties among the N * N candidates are plentiful.

Writes tests/golden/attn_decode_goldens.npz:
  names                      the case names; per case (prefix "<name>_"):
  beam, V, maxlen, sos, eos, steps ()       steps = decoder steps the reference took
  logits (steps, R, V) f32                  the mock decoder's output, R = beam
  tk_logp (steps, R, N) f32, tk_index (steps, R, N) i32   TopK(log_softmax(logits), N) before the finished-row masks
  scores_in / scores_out (steps, R) f32, end_in / end_out (steps, R) i32, tokens_in / tokens_out (steps, R, maxlen) i32
  parent (steps, R) i32, pred (steps, R) i32
  best_hyps (maxlen - 1,) i32, best_score () f32     recognize()'s result

usage: python tests/golden/gen_attn_decode_goldens.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_goldens import _load, load_reference  # noqa: E402


class _Tensor(np.ndarray):
    def __new__(cls, x, dtype=None):
        return np.asarray(x).view(cls)

    def asnumpy(self):
        return np.asarray(self)

    def view(self, *shape):
        if shape and all(isinstance(s, (int, np.integer)) for s in shape):
            return np.asarray(self).reshape(shape).view(_Tensor)
        return np.ndarray.view(self, *shape)


class Tables:
    """The logits function of a case."""

    def __init__(self, seed, V, maxlen, eos, quantum, eos_bias, sparse=False):
        rng = np.random.RandomState(seed)
        q = lambda x: (np.round(x / quantum) * quantum).astype(np.float32)  # noqa: E731
        self.V, self.eos, self.sparse = V, eos, sparse
        self.a1 = q(6.0 * rng.rand(V, V))
        self.a2 = q(6.0 * rng.rand(V, V))
        self.pos = q(4.0 * rng.rand(maxlen, V))
        self.bias = np.asarray([eos_bias(p) for p in range(maxlen)], np.float32)

    def logits(self, ids, t):
        """ids (R, >= t + 1) the rows' prefixes, t the position -> (R, V) float32."""
        last = ids[:, t]
        before = ids[:, t - 1] if t > 0 else np.zeros_like(last)
        g = self.a1[last] + np.float32(0.5) * self.a2[before] + self.pos[t][None, :]
        g = g.astype(np.float32)
        g[:, self.eos] += self.bias[t]
        top = g.max(1, keepdims=True)
        first = np.argmax(g, 1)
        out = (-(np.float32(30.0) + (top - g))).astype(np.float32)
        out[np.arange(len(ids)), first] = 0.0
        if self.sparse:  # a vocabulary mask: -inf logits (log_softmax stays the identity: exp(-inf) is 0)
            if t == 0:   # two finite tokens for a beam of four: two rows of the beam are dead (-inf) after the first step
                keep = np.argsort(-out, 1, kind="stable")[:, :2]
            else:        # a row that has not finished continues with its best token only
                keep = first[:, None]
            masked = np.full_like(out, -np.inf)
            np.put_along_axis(masked, keep, np.take_along_axis(out, keep, 1), 1)
            out = np.where((last == self.eos)[:, None] & (t > 0), out, masked)
        return out


class _Model:
    def __init__(self, rec, tables, beam, maxlen, eos):
        self.rec, self.tables, self.beam, self.maxlen, self.eos = rec, tables, beam, maxlen, eos
        self.steps = []
        enc = types.SimpleNamespace(encoder=lambda xs, m1, m2: (_Tensor(np.zeros((1, maxlen, 4), np.float32)),
                                                                _Tensor(np.ones((1, 1, maxlen), np.float32))))
        self.predict_network = types.SimpleNamespace(backbone=types.SimpleNamespace(acc_net=enc),
                                                     add_flags_recursive=lambda **kw: None)

    def predict(self, memory, memory_mask, tgt, tgt_mask, valid_length, end_flag, scores, base_index):
        rec, n = self.rec, self.beam
        tgt = np.asarray(tgt).astype(np.int32)
        vl = int(np.asarray(valid_length))
        end_flag = np.asarray(end_flag).astype(np.float32)
        scores = np.asarray(scores).astype(np.float32)
        if self.steps:  # what recognize() made of the previous step's outputs
            assert np.array_equal(tgt, self.steps[-1]["tokens_out"]) and np.array_equal(end_flag[:, 0], self.steps[-1]["end_out"])
        # decoder + log_softmax in float32 (372-385); the gather at valid_length is the position argument
        logits = self.tables.logits(tgt, vl)
        m = logits.max(1, keepdims=True)
        y = ((logits - m) - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
        assert np.array_equal(y, logits), "log_softmax must be the identity on these logits"
        # 2.2 (387-392)
        top_k_logp, top_k_index = rec.topk_fun(y, n)
        top_k_logp, top_k_index = top_k_logp.astype(np.float32), top_k_index.astype(np.int32)
        raw_logp, raw_index = top_k_logp.copy(), top_k_index.copy()
        top_k_logp = rec.mask_finished_scores(top_k_logp, end_flag).astype(np.float32)
        top_k_index = rec.mask_finished_preds(top_k_index, end_flag, self.eos)
        batch_size = top_k_logp.shape[0] // n
        # 2.3 (395-398)
        cand = (scores + top_k_logp).astype(np.float32).reshape(batch_size, n * n)
        new_scores, offset_k_index = rec.topk_fun(cand, n)
        new_scores = new_scores.astype(np.float32).reshape(-1, 1)
        # 2.4 (403-405)
        base_k_index = np.tile(np.asarray(base_index), (1, n)) * n * n
        best_k_index = base_k_index.reshape(-1) + offset_k_index.reshape(-1)
        # 2.5 (408-413)
        best_k_pred = top_k_index.reshape(-1)[best_k_index]
        best_hyps_index = best_k_index // n
        last_best_k_hyps = tgt[best_hyps_index]
        tokens_out = last_best_k_hyps.copy()
        tokens_out[:, vl + 1] = best_k_pred
        self.steps.append({"logits": logits, "tk_logp": raw_logp, "tk_index": raw_index, "scores_in": scores[:, 0].copy(),
                           "end_in": end_flag[:, 0].astype(np.int32), "tokens_in": tgt.copy(), "scores_out": new_scores[:, 0].copy(),
                           "end_out": (best_k_pred == self.eos).astype(np.int32), "tokens_out": tokens_out,
                           "parent": best_hyps_index.astype(np.int32), "pred": best_k_pred.astype(np.int32), "cand": cand[0].copy()})
        return (_Tensor(last_best_k_hyps), _Tensor(np.asarray(vl + 1)), _Tensor(end_flag), _Tensor(new_scores), _Tensor(best_k_pred))


# name: (beam, V, maxlen, quantum, eos bias by position, what the case must show).  beam4, length_limit and all_finish_step1 share the
# beam and the vocabulary (one eos), and length_limit has the largest maxlen of the three: they also run as one batch.
CASES = {
    "beam1": (1, 17, 14, 0.125, lambda p: -3.0 + 0.75 * p, None),
    "beam4": (4, 21, 21, 0.125, lambda p: -4.0 + 0.5 * p, "staggered"),
    "beam10": (10, 37, 40, 0.125, lambda p: -5.0 + 0.25 * p, "staggered"),
    "beam16": (16, 50, 26, 0.125, lambda p: -5.0 + 0.5 * p, "staggered"),
    "v_eq_beam10": (10, 10, 18, 0.125, lambda p: -4.0 + 0.5 * p, None),
    "v_eq_beam16": (16, 16, 12, 0.125, lambda p: -4.0 + 0.75 * p, None),
    "length_limit": (4, 21, 21, 0.125, lambda p: -1000.0, "limit"),
    "all_finish_first_step": (1, 16, 9, 0.125, lambda p: 1000.0, "first"),
    "all_finish_step1": (4, 21, 12, 0.125, lambda p: -1000.0 if p == 0 else 1000.0, "step1"),
    "ties": (10, 16, 16, 1.0, lambda p: -3.0 + 1.0 * p, "ties"),
    # eos first and one other finite token at step 0, then one finite token per unfinished row: fewer than N candidates are finite and
    # free of -10000, so the finished row's -10000 branches enter the beam ahead of the -inf candidates
    "neg10000_in_beam": (4, 19, 8, 0.125, lambda p: 1000.0 if p == 0 else -3.0 + 1.5 * p, "neg10000"),
    "maxlen2": (4, 18, 2, 0.125, lambda p: -2.0, None),
    "maxlen3": (10, 18, 3, 0.125, lambda p: 2.0 * p, None),
}


def main():
    load_reference()
    rec = _load("mindaudio.utils.recognize", "mindaudio/utils/recognize.py")
    rec.Tensor = _Tensor
    out = {"names": np.array(sorted(CASES))}
    for k, name in enumerate(sorted(CASES)):
        beam, V, maxlen, quantum, bias, show = CASES[name]
        sos = eos = V - 1
        model = _Model(rec, Tables(20261021 + k, V, maxlen, eos, quantum, bias, sparse=show == "neg10000"), beam, maxlen, eos)
        start_token = np.array([sos], np.int32)
        scores = np.array([0.0] + [-float("inf")] * (beam - 1), np.float32)
        end_flag = np.array([0.0] * beam, np.float32)
        base_index = np.arange(1, dtype=np.int32).reshape(-1, 1)
        best_hyps, best_scores = rec.recognize(model, np.zeros((1, 4 * maxlen + 8, 2)), np.ones((1, 1, 4 * maxlen + 8)), start_token,
                                               base_index, scores, end_flag, beam, eos, None, full_graph=False)
        st = model.steps
        assert best_hyps.shape == (1, maxlen - 1) and 1 <= len(st) <= maxlen - 1
        if show == "staggered":  # beams finish at different steps: the search goes on with some beams finished
            assert sum(0 < s["end_in"].sum() < beam for s in st) >= 2, name
        elif show == "limit":
            assert len(st) == maxlen - 1 and not any(s["end_out"].any() for s in st), name
        elif show == "first":
            assert len(st) == 1 and st[0]["end_out"].all(), name
        elif show == "step1":
            assert len(st) == 2 and not st[0]["end_out"].any() and st[1]["end_out"].all(), name
        elif show == "neg10000":
            assert any((s["scores_out"] < -5000).any() and np.isfinite(s["scores_out"]).all() for s in st), name
            assert np.isneginf(st[0]["scores_out"]).sum() == 2 and not any(np.isnan(s["scores_out"]).any() for s in st), name
        elif show == "ties":  # an exact tie across the beam's edge, and one inside the beam
            edge = inside = 0
            for s in st:
                c = np.sort(s["cand"][np.isfinite(s["cand"])])[::-1]
                if len(c) > beam:
                    edge += int(c[beam - 1] == c[beam])
                    inside += int((c[:beam - 1] == c[1:beam]).any())
            assert edge >= 1 and inside >= 1, (name, edge, inside)
        p = name + "_"
        out.update({p + "beam": np.int32(beam), p + "V": np.int32(V), p + "maxlen": np.int32(maxlen), p + "sos": np.int32(sos),
                    p + "eos": np.int32(eos), p + "steps": np.int32(len(st)),
                    p + "best_hyps": np.asarray(best_hyps[0], np.int32), p + "best_score": np.float32(np.asarray(best_scores).reshape(-1)[0])})
        for key in ("logits", "tk_logp", "tk_index", "scores_in", "end_in", "tokens_in", "scores_out", "end_out", "tokens_out",
                    "parent", "pred"):
            out[p + key] = np.stack([s[key] for s in st])
        print("%-22s beam %2d V %2d maxlen %2d steps %2d best %s %.3f" % (name, beam, V, maxlen, len(st), best_hyps[0].tolist(),
                                                                          float(out[p + "best_score"])))
    path = os.path.join(HERE, "attn_decode_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
