"""Cases, float64 restatements and comparators of the autoregressive `attention` decode mode (csrc/attn_decode.hip,
TransformerDecoder.init_cache / step, conformer.asr_model.recognize).  NumPy only: tests/test_attn_decode_cases_cpu.py proves this file
without a device, tests/test_attn_decode_gpu.py holds the kernels to it.

Restatements:
  decoder_full / decoder_step   the Transformer decoder in float64: as the reference runs a step (the full maxlen-padded prefix, the
                                padded subsequent mask, then the gather of row valid_length - recognize.py:187-226,
                                decoder_factory.py:372-380) and on a key / value cache.  `rnd` is applied where the device rounds to
                                bf16 (below); with rnd = ident they are exact.
  beam_step                     steps 2.2-2.6 (decoder_factory.py:387-413, recognize.py:236-242) with the frozen-utterance rule
  search                        the whole loop for one utterance on any logits source
Every restatement takes `defect=`: a planted error that the comparators must reject.

bf16 rounding points of the device path (ops.gemm / ops.layernorm / the attention kernels): the matmul weights; the encoder output;
every LayerNorm output; the q | k | v, source-attention q and k | v, and ReLU(w_1) GEMM outputs; the normalised attention
probabilities; the attention context.  The residual stream, biases, LayerNorm parameters, the embedding and the logits are float32.

GUARD: the end-to-end cases (E2E) compare token decisions of the device with the float64 search, which is only meaningful where no
decision is closer than the arithmetic's noise.  A case is kept when the float64 search's smallest decision gap (between the N-th and
(N+1)-th candidate, and between neighbours inside the first N; exact ties between candidates of finished rows' -10000 branches do not
occur inside the first N + 1 of a kept case) stays above GUARD at every step.  GUARD = 4 x the largest candidate-score difference
that the bf16-rounded restatement shows against float64 along the float64 search's path on those cases: measured 0.0822 (see
test_guard_is_four_times_the_rounding_noise, which measures it again), so GUARD = 0.33.  Six of the eight cases are kept (beam 1
and 2); the beam 3 and beam 4 cases have decisions closer than the guard and are not compared."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NEG = -10000.0
GUARD = 0.33
GUARD_MEASURED = 0.0822  # largest |bf16-rounded - float64| candidate score over the E2E cases

# ---- case tables ---------------------------------------------------------------------------------------------------------------------
# ma_decoder_self_attn_step_bf16: (R, Lmax); heads 4
STEP_SHAPES = ((1, 9), (4, 9), (10, 70), (48, 70))
STEP_T = (0, 1, 31, 32, 33, 63, 64)  # and Lmax - 1


def step_ts(lmax):
    return sorted({t for t in STEP_T + (lmax - 1,) if t < lmax})


# the smallest model the constructors take
D, HEADS, BLOCKS, UNITS = 256, 4, 2, 64
# end to end: (seed, V, beam, encoder frames)
E2E = ((255, 33, 1, 10), (24, 16, 1, 9), (393, 23, 2, 12), (285, 27, 2, 11), (29, 27, 2, 11), (145, 23, 2, 12), (10, 31, 3, 10),
       (44, 19, 4, 9))
E2E_OUT_GAIN, E2E_EOS_BIAS = 6.0, 4.0  # a peaky output layer and an eos that wins now and then: beams finish, gaps are wide
# TransformerDecoder.step against the restatement: (V, rows, group, encoder frames), steps checked
STEP_MODEL = (37, 6, 3, 40)
STEP_MODEL_TS = (1, 2, 33, 39)


def goldens():
    return np.load(os.path.join(HERE, "golden", "attn_decode_goldens.npz"))


def golden_names(g):
    return [str(n) for n in g["names"]]


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
def ident(x):
    return x


def bf16(x):
    """Round to the nearest bf16 (ties to even), returned as float64."""
    f = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = u.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(np.isfinite(f), out, f.astype(np.float64))


def relrms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((a - ref) ** 2) / np.mean(ref ** 2)))


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def sinusoid(max_len, d):
    """layers/embedding.py:36-44, in the float32 arithmetic of the model's table."""
    pos = np.arange(max_len, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * -(math.log(10000.0) / d))
    pe = np.zeros((max_len, d))
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe.astype(np.float32).astype(np.float64)


def random_weights(seed, vocab, d=D, units=UNITS, blocks=BLOCKS, out_gain=1.0, eos_bias=0.0):
    """float32-valued decoder parameters under the reference's parameter layout (a state dict of TransformerDecoder)."""
    rng = np.random.RandomState(seed)
    lin = lambda o, i, g=1.0: ((g * rng.randn(o, i) / np.sqrt(i)).astype(np.float32), (0.1 * rng.randn(o)).astype(np.float32))  # noqa: E731
    sd = {"embed.weight": (rng.randn(vocab, d) / np.sqrt(d)).astype(np.float32) * np.float32(4.0)}
    for n in range(blocks):
        p = "decoders.%d." % n
        for att in ("self_attn", "src_attn"):
            for name in ("linear_q", "linear_k", "linear_v", "linear_out"):
                g = 2.0 if name in ("linear_q", "linear_k") else 1.0
                sd[p + att + "." + name + ".weight"], sd[p + att + "." + name + ".bias"] = lin(d, d, g)
        sd[p + "feed_forward.w_1.weight"], sd[p + "feed_forward.w_1.bias"] = lin(units, d)
        sd[p + "feed_forward.w_2.weight"], sd[p + "feed_forward.w_2.bias"] = lin(d, units)
        for ln in ("norm1", "norm2", "norm3"):
            sd[p + ln + ".gamma"] = (1.0 + 0.1 * rng.randn(d)).astype(np.float32)
            sd[p + ln + ".beta"] = (0.1 * rng.randn(d)).astype(np.float32)
    sd["after_norm.gamma"] = (1.0 + 0.1 * rng.randn(d)).astype(np.float32)
    sd["after_norm.beta"] = (0.1 * rng.randn(d)).astype(np.float32)
    sd["output_layer.weight"], sd["output_layer.bias"] = lin(vocab, d, out_gain)
    sd["output_layer.bias"][vocab - 1] += np.float32(eos_bias)
    return sd


class Decoder:
    """The float64 restatement on a state dict.  rnd = ident: exact; rnd = bf16: rounded where the device rounds."""

    def __init__(self, sd, heads=HEADS, rnd=ident, max_len=64):
        self.rnd, self.heads = rnd, heads
        self.sd = {k: (rnd(np.asarray(v, np.float64)) if k.endswith(".weight") and not k.startswith("embed") else np.asarray(v, np.float64))
                   for k, v in sd.items()}
        self.d = self.sd["embed.weight"].shape[1]
        self.blocks = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("decoders."))
        self.pe = sinusoid(max_len, self.d)

    def lin(self, x, name):
        return x @ self.sd[name + ".weight"].T + self.sd[name + ".bias"]

    def ln(self, x, name):
        m = x.mean(-1, keepdims=True)
        v = ((x - m) ** 2).mean(-1, keepdims=True)
        return self.rnd((x - m) / np.sqrt(v + 1e-12) * self.sd[name + ".gamma"] + self.sd[name + ".beta"])

    def attend(self, q, k, v, mask):
        """q (R, Lq, d), k / v (R, Lk, d), mask (R, Lq, Lk) bool or None -> (R, Lq, d); scores / d_k (q and k both carry 1/sqrt(d_k))."""
        r, lq, d = q.shape
        h, dk = self.heads, d // self.heads
        qh, kh, vh = (x.reshape(r, -1, h, dk).transpose(0, 2, 1, 3) for x in (q, k, v))
        s = qh @ kh.transpose(0, 1, 3, 2) / dk
        if mask is not None:
            s = s + np.where(mask[:, None], 0.0, NEG)
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p = self.rnd(p / p.sum(-1, keepdims=True))
        return self.rnd((p @ vh).transpose(0, 2, 1, 3).reshape(r, lq, d))

    def embed(self, ids, pos):
        return self.sd["embed.weight"][ids] * np.sqrt(self.d) + self.pe[pos]

    def memory_kv(self, memory):
        m = self.rnd(np.asarray(memory, np.float64))
        return [(self.rnd(self.lin(m, "decoders.%d.src_attn.linear_k" % n)), self.rnd(self.lin(m, "decoders.%d.src_attn.linear_v" % n)))
                for n in range(self.blocks)]

    def _rest(self, n, x, mk, mv, mem_mask):
        p = "decoders.%d." % n
        a = self.ln(x, p + "norm2")
        q = self.rnd(self.lin(a, p + "src_attn.linear_q"))
        mm = None if mem_mask is None else np.broadcast_to(mem_mask[:, None, :], (x.shape[0], x.shape[1], mk.shape[1]))
        x = x + self.lin(self.attend(q, mk, mv, mm), p + "src_attn.linear_out")
        a = self.ln(x, p + "norm3")
        hdn = self.rnd(np.maximum(self.lin(a, p + "feed_forward.w_1"), 0.0))
        return x + self.lin(hdn, p + "feed_forward.w_2")

    def full(self, memory, mem_mask, ids, self_mask):
        """memory (R, T', d), mem_mask (R, T') bool or None, ids (R, L), self_mask (L, L) bool -> logits (R, L, V)."""
        r, l = ids.shape
        x = self.embed(ids, np.arange(l))
        kv = self.memory_kv(memory)
        sm = np.broadcast_to(self_mask[None], (r, l, l))
        for n in range(self.blocks):
            p = "decoders.%d." % n
            a = self.ln(x, p + "norm1")
            q, k, v = (self.rnd(self.lin(a, p + "self_attn.linear_" + c)) for c in "qkv")
            x = x + self.lin(self.attend(q, k, v, sm), p + "self_attn.linear_out")
            x = self._rest(n, x, kv[n][0], kv[n][1], mem_mask)
        return self.lin(self.ln(x, "after_norm"), "output_layer")

    def reference_step(self, memory, mem_mask, ids_padded, i):
        """Step i (1-based) as the reference runs it: the maxlen-padded prefix, subsequent_mask(i) padded with False to maxlen, then
        row valid_length = i - 1 (rows whose mask line is all False see a uniform softmax; they are never gathered)."""
        maxlen = ids_padded.shape[1]
        m = np.zeros((maxlen, maxlen), bool)
        m[:i, :i] = np.tril(np.ones((i, i), bool))
        return self.full(memory, mem_mask, ids_padded, m)[:, i - 1]

    def init_cache(self, memory, mem_mask, group, max_len):
        """memory (B, T', d) of B utterances, `group` rows each: the source K / V once per utterance."""
        b = memory.shape[0]
        return {"kv": self.memory_kv(memory), "mask": mem_mask, "group": group,
                "k": [np.zeros((b * group, max_len, self.d)) for _ in range(self.blocks)],
                "v": [np.zeros((b * group, max_len, self.d)) for _ in range(self.blocks)]}

    def step(self, cache, tokens, t, parent=None, defect=None):
        """tokens (R,), t cached positions, parent (R,) or None -> logits (R, V); the cache is reordered and extended."""
        r = len(tokens)
        par = np.arange(r) if parent is None else np.asarray(parent)
        g = cache["group"]
        x = self.embed(np.asarray(tokens), t)[:, None, :]
        for n in range(self.blocks):
            p = "decoders.%d." % n
            a = self.ln(x, p + "norm1")
            q, k, v = (self.rnd(self.lin(a, p + "self_attn.linear_" + c)) for c in "qkv")
            cache["k"][n], cache["v"][n] = cache_update(cache["k"][n], cache["v"][n], k[:, 0], v[:, 0], par, t, defect)
            x = x + self.lin(self.attend(q, cache["k"][n][:, :t + 1], cache["v"][n][:, :t + 1], None), p + "self_attn.linear_out")
            mk, mv = (np.repeat(m, g, 0) for m in cache["kv"][n])
            mm = None if cache["mask"] is None else np.repeat(cache["mask"], g, 0)
            x = self._rest(n, x, mk, mv, mm)
        return self.lin(self.ln(x, "after_norm"), "output_layer")[:, 0]


def cache_update(k_in, v_in, k_new, v_new, parent, t, defect=None):
    """The cache rule of ma_decoder_self_attn_step_bf16: out[r, :t] = in[parent[r], :t], out[r, t] = the new row; rows above t keep
    what the out buffer held (here: a copy of the in buffer's).  Defects: "copy_self" copies from r, "no_append" leaves row t."""
    src = np.arange(len(parent)) if defect == "copy_self" else parent
    k_out, v_out = k_in.copy(), v_in.copy()
    k_out[:, :t], v_out[:, :t] = k_in[src, :t], v_in[src, :t]
    if defect != "no_append":
        k_out[:, t], v_out[:, t] = k_new, v_new
    return k_out, v_out


def self_attn_step(qkv, k_in, v_in, parent, t, heads, scale, defect=None):
    """ma_decoder_self_attn_step_bf16 in float64 on the values given, with the kernel's two roundings (probabilities, context):
    -> (ctx (R, d), k_out, v_out)."""
    r, d = qkv.shape[0], qkv.shape[1] // 3
    par = np.arange(r) if parent is None else np.asarray(parent)
    k_out, v_out = cache_update(k_in, v_in, qkv[:, d:2 * d], qkv[:, 2 * d:], par, t, defect)
    dk = d // heads
    q = qkv[:, :d].reshape(r, heads, 1, dk)
    kh = k_out[:, :t + 1].reshape(r, t + 1, heads, dk).transpose(0, 2, 1, 3)
    vh = v_out[:, :t + 1].reshape(r, t + 1, heads, dk).transpose(0, 2, 1, 3)
    s = (q @ kh.transpose(0, 1, 3, 2)) * scale
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = bf16(p / p.sum(-1, keepdims=True))
    return bf16((p @ vh).reshape(r, d)), k_out, v_out


def hadamard64():
    h = np.array([[1.0]])
    for _ in range(6):
        h = np.block([[h, h], [h, -h]])
    return h


class OneHot:
    """Exact cases of the step kernel for one (R, Lmax).  Key (p, j) is 8 s_j u_{j % 64} + n(p, j) per head - u the rows of the
    64 x 64 Hadamard matrix, s_j = +1 below position 64 and -1 from there on, n a row-dependent multiple of 1/16 in [-1/4, 1/4] that
    makes every cache row distinct (all exact in bf16) - and row r's query is 16 s u of its target position (r + shift) % (t + 1):
    the target scores 128 +- 4, every other key at most 4 in magnitude, so the target's weight is exactly 1 and ctx[r] is the value
    row (parent[r], target) - or row r's new value when the target is t - bit for bit.  parent[r] = (r + shift) % R: every parent and
    every position are hit as `shift` runs.  k_in / v_in (R, Lmax, d) are the cache, k_new / v_new (R, Lmax, d) what row r appends
    when the step is t (position t of the in cache holds other values: a real cache holds anything there)."""

    def __init__(self, R, lmax, heads=HEADS, seed=0):
        rng = np.random.RandomState(seed * 1009 + R * 131 + lmax * 17)
        d = heads * 64
        had = hadamard64()
        pat = np.stack([np.tile((8.0 if j < 64 else -8.0) * had[j % 64], heads) for j in range(lmax)])      # (lmax, d)
        noise = lambda: rng.randint(-4, 5, size=(R, lmax, d)) / 16.0  # noqa: E731
        value = lambda: bf16(rng.randn(R, lmax, d) + 3.0 * np.sign(rng.randn(R, lmax, d)))  # noqa: E731  (no zeros: -0 + 0 loses its sign)
        f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
        self.R, self.lmax, self.d, self.heads = R, lmax, d, heads
        self.k_in, self.k_new, self.v_in, self.v_new = f(pat[None] + noise()), f(pat[None] + noise()), f(value()), f(value())
        self.q_pat = f(2.0 * pat)

    def case(self, t, shift):
        """-> (qkv (R, 3 d) float32 of bf16 values, parent (R,) int32, want_ctx (R, d), want_k, want_v (R, t + 1, d))."""
        R = self.R
        target = (np.arange(R) + shift) % (t + 1)
        parent = ((np.arange(R) + shift) % R).astype(np.int32)
        qkv = np.concatenate([self.q_pat[target], self.k_new[:, t], self.v_new[:, t]], 1)
        want_k, want_v = cache_update(self.k_in, self.v_in, self.k_new[:, t], self.v_new[:, t], parent, t)
        return qkv, parent, want_v[np.arange(R), target], want_k[:, :t + 1], want_v[:, :t + 1]


# ---- the beam step -------------------------------------------------------------------------------------------------------------------
def topk_rows(logp, n):
    """The n best per row, descending, equal values lower index first (ma_ctc_topk_f32 / the reference's stable topk_fun)."""
    order = np.stack([np.lexsort((np.arange(logp.shape[1]), -row))[:n] for row in logp])
    return np.take_along_axis(logp, order, 1), order.astype(np.int32)


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def beam_candidates(tk_logp, scores, end, dtype=np.float64, defect=None):
    """The N * N candidate values of one utterance (rows, N), in `dtype`."""
    lp = np.asarray(tk_logp, dtype)
    n = lp.shape[1]
    fin = np.asarray(end).astype(bool)[:, None]
    neg = dtype(-np.inf) if defect == "neg_inf" else dtype(NEG)
    first = np.arange(n)[None, :] == 0
    m = np.where(fin, np.where(first, lp if defect == "no_zero" else dtype(0.0), lp + neg), lp).astype(dtype)
    return (np.asarray(scores, dtype)[:, None] + m).astype(dtype)


def beam_step(tk_logp, tk_index, scores, end, tokens, length, done, eos, max_new, dtype=np.float64, defect=None):
    """One utterance (rows = N): -> (scores_out, end_out, tokens_out, parent (local row), pred, length, done, candidates)."""
    n = tk_logp.shape[0]
    tokens = np.asarray(tokens)
    if done:
        return (np.asarray(scores, dtype).copy(), np.asarray(end, np.int32).copy(), tokens.copy(), np.arange(n, dtype=np.int32),
                np.full(n, eos, np.int32), length + (1 if defect == "frozen_length" else 0), 1, None)
    cand = beam_candidates(tk_logp, scores, end, dtype, defect)
    flat = cand.reshape(-1)
    key = np.where(np.isnan(flat), -np.inf, flat)
    tie = -np.arange(n * n) if defect == "ties_high" else np.arange(n * n)
    order = np.lexsort((tie, -key))[:n]
    tok = np.where(np.asarray(end).astype(bool)[:, None], eos, np.asarray(tk_index)).reshape(-1)[order].astype(np.int32)
    parent = (order // n).astype(np.int32)
    tokens_out = tokens[parent].copy()
    tokens_out[:, length + 1] = tok
    end_out = (tok == eos).astype(np.int32)
    length += 1
    return flat[order], end_out, tokens_out, parent, tok, length, int(end_out.all() or length >= max_new), cand


def decision_gap(cand, n, scores=None, end=None, logp=None):
    """The smallest gap between neighbours among the best n + 1 candidates (the ranks that decide the step's outcome).  With the
    step's full log-probabilities (rows, V) the candidates are score[r] + logp[r][v] over EVERY token v of the unfinished rows (the
    top-k lists hide the (n + 1)-th token of a row) plus the finished rows' branches."""
    if logp is not None:
        fin = np.asarray(end).astype(bool)
        cand = np.concatenate([(np.asarray(scores)[:, None] + logp)[~fin].reshape(-1), cand[fin].reshape(-1)])
    flat = np.sort(cand.reshape(-1))[::-1][:n + 1]
    flat = flat[np.isfinite(flat)]
    return float(np.min(flat[:-1] - flat[1:])) if len(flat) > 1 else np.inf


def search(step_logits, beam, maxlen, sos, eos, dtype=np.float64, defect=None, on_step=None):
    """recognize() for one utterance: step_logits(tokens (N,), t, parent or None) -> logits (N, V) -> dict(best_hyps (maxlen - 1,),
    best_score, length, min_gap, steps).  log_softmax and the top-k are taken in `dtype`."""
    scores = np.array([0.0] + [-np.inf] * (beam - 1), dtype)
    end = np.zeros(beam, np.int32)
    tokens = np.zeros((beam, maxlen), np.int32)
    tokens[:, 0] = sos
    length, done, parent, last, gap, steps = 0, int(maxlen - 1 < 1), None, tokens[:, 0].copy(), np.inf, 0
    while not done:
        logits = np.asarray(step_logits(last, length, parent), dtype)
        full = log_softmax(logits).astype(dtype)
        lp, ix = topk_rows(full, beam)
        t, before = length, (scores, end)
        scores, end, tokens, parent, last, length, done, cand = beam_step(lp, ix, scores, end, tokens, length, done, eos, maxlen - 1,
                                                                          dtype, defect)
        gap = min(gap, decision_gap(cand, beam, before[0], before[1], full))
        steps += 1
        if on_step is not None:
            on_step(t, cand, before + (parent, last))
    best = int(np.argmax(np.where(np.isnan(scores), -np.inf, scores)))  # (the first of equal maxima)
    return {"best_hyps": tokens[best, 1:].copy(), "best_score": scores[best], "length": length, "min_gap": gap, "steps": steps}


def e2e_inputs(seed, vocab, frames):
    rng = np.random.RandomState(1000 + seed)
    memory = rng.randn(1, frames, D).astype(np.float32)
    mask = np.ones((1, frames), bool)
    mask[0, frames - 2:] = seed % 2 == 0  # (every other case has two padded encoder frames)
    return memory, mask


def e2e_reference(seed, vocab, beam, frames):
    """The float64 search of an end-to-end case on the KV-cached restatement, with the bf16-rounded restatement run along the same
    path: -> (state dict, memory, mask, result dict of `search` + "noise").  noise = the largest difference of a candidate score
    (score[r] + logp[r][v] over every live unfinished row r and EVERY token v; the score alone for a finished row) between the two,
    the rounded one accumulating its own scores along the float64 search's choices."""
    sd = random_weights(seed, vocab, out_gain=E2E_OUT_GAIN, eos_bias=E2E_EOS_BIAS)
    d64, dbf = Decoder(sd), Decoder(sd, rnd=bf16)
    memory, mask = e2e_inputs(seed, vocab, frames)
    c64, cbf = (d.init_cache(memory.astype(np.float64), mask, beam, frames) for d in (d64, dbf))
    noise, sb, state = [0.0], [np.array([0.0] + [-np.inf] * (beam - 1))], {}

    def logits(tok, t, par):
        state["l64"] = log_softmax(d64.step(c64, tok, t, par))
        state["lbf"] = log_softmax(dbf.step(cbf, tok, t, par))
        return state["l64"]

    def on_step(t, cand, info):
        scores, end, parent, tok = info
        live = np.isfinite(scores)
        fin = end.astype(bool)
        c64_, cbf_ = scores[:, None] + state["l64"], sb[0][:, None] + state["lbf"]
        if (live & ~fin).any():
            noise[0] = max(noise[0], float(np.abs(cbf_[live & ~fin] - c64_[live & ~fin]).max()))
        if (live & fin).any():
            noise[0] = max(noise[0], float(np.abs(sb[0][live & fin] - scores[live & fin]).max()))
        sb[0] = np.where(fin[parent], sb[0][parent], sb[0][parent] + state["lbf"][parent, tok])

    res = search(logits, beam, frames, vocab - 1, vocab - 1, on_step=on_step)
    res["noise"] = noise[0]
    return sd, memory, mask, res


# ---- comparators -----------------------------------------------------------------------------------------------------------------------
def check_cache(got_k, got_v, want_k, want_v, t):
    """Rows 0..t of the out cache, bit for bit (arrays of bf16 values as float32 / float64)."""
    for name, got, want in (("k", got_k, want_k), ("v", got_v, want_v)):
        got, want = np.asarray(got, np.float64)[:, :t + 1], np.asarray(want, np.float64)[:, :t + 1]
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s cache differs at (row, position, column) %s" % (name, bad[0].tolist())


def check_ctx_exact(got, want):
    bad = np.argwhere(np.asarray(got, np.float32).view(np.uint32) != np.asarray(want, np.float32).view(np.uint32))
    assert bad.size == 0, "ctx differs at (row, column) %s" % bad[0].tolist()


def check_ctx_close(got, want, v_used):
    """|err| <= 2^-7 max|v| per row: the probabilities and the output are each rounded to bf16 (2^-9 relative each; the device's
    rounding may flip against the restatement's), float32 sums over at most 256 terms are far below that; the margin is 2 x."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = 2.0 ** -7 * np.abs(v_used).reshape(len(got), -1).max(1)
    err = np.abs(got - want).max(1)
    assert (err <= bound).all(), "ctx row %d: |err| %.3g > %.3g" % (int(np.argmax(err / bound)), err.max(), bound[int(np.argmax(err / bound))])


def check_beam(got, want, exact_scores=True):
    """(scores_out, end_out, tokens_out, parent, pred, length, done) of one utterance."""
    names = ("scores_out", "end_out", "tokens_out", "parent", "pred", "length", "done")
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name == "scores_out":
            same = np.array_equal(g.astype(np.float32).view(np.uint32), w.astype(np.float32).view(np.uint32)) if exact_scores else \
                np.allclose(g, w, rtol=1e-6, atol=0, equal_nan=True)
            # (+0.0 and -0.0 are one score)
            same = same or np.array_equal(g.astype(np.float32), w.astype(np.float32))
            assert same, "scores_out: %s != %s" % (g, w)
        else:
            assert np.array_equal(g, w), "%s: %s != %s" % (name, g.tolist(), w.tolist())


def golden_step(g, name, s):
    """Inputs and expected outputs of recorded step s of a golden case."""
    p = name + "_"
    ins = {k: g[p + k][s] for k in ("tk_logp", "tk_index", "scores_in", "end_in", "tokens_in")}
    n, maxlen, steps = int(g[p + "beam"]), int(g[p + "maxlen"]), int(g[p + "steps"])
    done = int(g[p + "end_out"][s].all() or s + 1 >= maxlen - 1)
    want = (g[p + "scores_out"][s], g[p + "end_out"][s], g[p + "tokens_out"][s], g[p + "parent"][s], g[p + "pred"][s], s + 1, done)
    assert done == int(s == steps - 1)  # the reference stopped exactly where `done` says
    return ins, want, n, maxlen
