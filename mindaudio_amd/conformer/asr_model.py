"""Mirror of examples/conformer/asr_model.py — forward / evaluation loss on MI355X, pure CTC (ctc_weight = 1.0, decoder None:
asr_model.py:327-328) and the hybrid CTC / attention configuration of the shipped conformer.yaml.

ASRModel.forward takes the 11 columns of the reference batch in the reference order (train.py:38-50) and returns
(loss, acc_att) like ASRModelWithAcc.construct (asr_model.py:75-153)."""
import torch
import torch.nn as nn

from .. import _host, ops
from ..models.conformer import ConformerEncoder


class CTC(nn.Module):
    """mindaudio/loss/ctc_loss.py:10-64: Dense(eprojs -> odim), float32 log_softmax, CTCLossV2(blank 0,
    zero_infinity), sum / batch."""

    def __init__(self, odim, encoder_output_size, dropout_rate=0.0, compute_type=None):
        super().__init__()
        self.ctc_lo = nn.Linear(encoder_output_size, odim)
        self._w = None
        self.register_load_state_dict_post_hook(lambda module, _keys: setattr(module, "_w", None))  # stale bf16 copy

    @torch.no_grad()
    def prepare(self):
        self._w = (self.ctc_lo.weight.detach().to(torch.bfloat16).contiguous(),
                   self.ctc_lo.bias.detach().float().contiguous())
        return self

    @torch.no_grad()
    def logits(self, hs_pad):
        if self._w is None:
            self.prepare()
        b, t, d = hs_pad.shape
        a = ops.cast_bf16(hs_pad.reshape(b * t, d).contiguous())
        return ops.gemm(a, self._w[0], bias=self._w[1], out_dtype=torch.float32)

    @torch.no_grad()
    def forward(self, hs_pad, hlens, ys_pad, ys_lengths):
        b, t, _ = hs_pad.shape
        loss, _ = ops.ctc_loss(self.logits(hs_pad), b, t, ys_pad, hlens, ys_lengths, blank=0, zero_infinity=True)
        return loss


class ASRModel(nn.Module):
    """Encoder + CTC [+ attention decoder] (asr_model.py:16-153).  forward() is the evaluation forward (create_asr_eval_net,
    asr_model.py:355-371) of either configuration: pure CTC (ctc_weight == 1.0) or the hybrid 0.3 / 0.7 loss with the
    TransformerDecoder and label smoothing; the training step (forward + backward + optimizer) is mindaudio_amd.train.engine."""

    def __init__(self, vocab_size, encoder, ctc, ctc_weight=1.0, decoder=None, lsm_weight=0.0, reverse_weight=0.0,
                 length_normalized_loss=False):
        super().__init__()
        if ctc_weight != 1.0 and decoder is None:
            raise ValueError("ctc_weight != 1.0 needs a decoder (asr_model.py:327-337)")
        if reverse_weight != 0.0:
            # asr_model.py:175-178 weighs in a right-to-left decoder's loss, but the reference ships no such decoder:
            # TransformerDecoder.construct returns a constant as r_decoder_out (models/conformer.py:606-639), so the
            # reference itself fails on reverse_weight > 0.  Same here, with a message.
            raise ValueError("reverse_weight > 0 needs a bidirectional decoder; the reference has none "
                             "(models/conformer.py:620, 639)")
        self.vocab_size, self.encoder, self.ctc, self.ctc_weight = vocab_size, encoder, ctc, ctc_weight
        self.decoder, self.lsm_weight = decoder, lsm_weight
        self.reverse_weight, self.length_normalized_loss = 0.0, bool(length_normalized_loss)

    @torch.no_grad()
    def forward(self, xs_pad, ys_pad, ys_in_pad=None, ys_out_pad=None, r_ys_in_pad=None, r_ys_out_pad=None,
                xs_masks=None, ys_sub_masks=None, ys_masks=None, ys_lengths=None, xs_chunk_masks=None):
        encoder_out, encoder_mask = self.encoder(xs_pad, xs_masks, xs_chunk_masks)
        # asr_model.py:109-114: lengths = mask.squeeze().sum(1) as int32
        encoder_out_lens = encoder_mask.to(torch.float32).reshape(encoder_mask.shape[0], -1).sum(1).to(torch.int32)
        loss_att = acc_att = None
        if self.ctc_weight != 1.0:  # attention-decoder branch (asr_model.py:117-129, 154-209)
            loss_att, acc_att = self._calc_att_loss(encoder_out, encoder_mask, ys_in_pad, ys_out_pad, ys_masks, ys_sub_masks)
        loss_ctc = self.ctc(encoder_out, encoder_out_lens, ys_pad, ys_lengths) if self.ctc_weight != 0.0 else None
        if loss_ctc is None:
            return loss_att, acc_att
        if loss_att is None:
            return loss_ctc, None
        return self.ctc_weight * loss_ctc + (1.0 - self.ctc_weight) * loss_att, acc_att  # asr_model.py:138-139

    @torch.no_grad()
    def _calc_att_loss(self, encoder_out, encoder_mask, ys_in_pad, ys_out_pad, ys_masks, ys_sub_masks):
        """asr_model.py:154-209: decoder scores -> LabelSmoothingLoss (KL, summed, / batch: label_smoothing_loss.py:24-117) and the
        token accuracy over the unmasked positions."""
        from ..train import kernels as K

        if ys_in_pad is None or ys_out_pad is None or ys_masks is None or ys_sub_masks is None:
            raise ValueError("the hybrid loss needs ys_in_pad, ys_out_pad, ys_sub_masks and ys_masks")
        scores, _ = self.decoder(encoder_out, encoder_mask, ys_in_pad, ys_sub_masks)
        b, l1, v = scores.shape
        logits = scores.reshape(b * l1, v)  # a view of the decoder's 64-padded row buffer
        tgt = ys_out_pad.to(torch.int32).contiguous().reshape(-1)
        tmask = ys_masks.to(torch.float32).contiguous().reshape(-1)
        stats, _ = K.label_smoothing_loss_grad(logits, v, tgt, tmask, self.lsm_weight, 0.0)
        # label_smoothing_loss.py:105-106: divided by the token count when normalize_length, else by the batch size
        return stats[0] / (stats[2] if self.length_normalized_loss else b), stats[1] / stats[2]


def create_asr_model(input_dim, vocab_size, encoder_conf=None, global_cmvn=None, ctc_weight=1.0, decoder_conf=None,
                     lsm_weight=0.0, length_normalized_loss=False):
    """creadte_asr_model (asr_model.py:301-352): decoder None when ctc_weight == 1.0, else a TransformerDecoder."""
    from ..models.decoder import TransformerDecoder

    encoder = ConformerEncoder(input_dim, global_cmvn=global_cmvn, **(encoder_conf or {}))
    ctc = CTC(vocab_size, encoder.output_size())
    decoder = None
    if ctc_weight != 1.0:
        decoder = TransformerDecoder(vocab_size, encoder.output_size(), **(decoder_conf or {}))
    return ASRModel(vocab_size, encoder, ctc, ctc_weight, decoder=decoder, lsm_weight=lsm_weight,
                    length_normalized_loss=length_normalized_loss)


class ASREvalNet(nn.Module):
    """create_asr_eval_net (asr_model.py:355-371): all-reduce (SUM) of the loss over the data-parallel ranks, divided
    by device_num.  One process per GPU; the collective is torch.distributed's (backend "nccl" = RCCL over xGMI on the
    GPU box, "gloo" in the CPU tests)."""

    def __init__(self, network, device_num):
        super().__init__()
        self.network, self.device_num = network, device_num

    @torch.no_grad()
    def forward(self, *inputs, **kwargs):
        out = self.network(*inputs, **kwargs)
        loss = out[0] if isinstance(out, tuple) else out
        loss = loss.clone().reshape(1)
        if self.device_num > 1:
            import torch.distributed as dist

            dist.all_reduce(loss, op=dist.ReduceOp.SUM)
        return loss[0] / self.device_num


def shard_batch(columns, rank, group_size):
    """Every rank builds the same global batch and keeps the strided slice batch[rank::group_size]
    (examples/conformer/dataset.py:552-553)."""
    return [c[rank::group_size] for c in columns]


def remove_duplicates_and_blank(hyp):
    """mindaudio/utils/common.py:116-125 on a host list (the device version lives in ma_ctc_greedy_search_f32)."""
    out, prev = [], None
    for tok in hyp:
        if tok != prev and tok != 0:
            out.append(tok)
        prev = tok
    return out


class CTCGreedySearch(nn.Module):
    """CTC greedy search net (models/decoders/decoder_factory.py:9-56): forward(xs_pad, xs_masks, xs_lengths) ->
    (topk_index (B, T') int32 with padded frames zeroed, topk_prob (B, T') float32 log-probabilities).
    `xs_masks` is the un-subsampled (B, 1, T) pad mask, sliced [:, :, :-2:2][:, :, :-2:2] here as in the reference."""

    def __init__(self, backbone, pretrained_model=False):
        super().__init__()
        if pretrained_model:
            raise NotImplementedError("wav2vec front ends are outside the built path")
        self.backbone = backbone

    @torch.no_grad()
    def forward(self, xs_pad, xs_masks, xs_lengths=None):
        best, logp, _, _ = self._search(xs_pad, xs_masks)
        return best, logp

    @torch.no_grad()
    def _search(self, xs_pad, xs_masks):
        sub = xs_masks[:, :, :-2:2][:, :, :-2:2].contiguous()
        enc, enc_mask = self.backbone.encoder(xs_pad, sub, sub)
        b, t2, _ = enc.shape
        logits = self.backbone.ctc.logits(enc)
        return ops.ctc_greedy_search(logits, b, t2, logits.shape[1], enc_mask.reshape(-1).to(torch.float32).contiguous())


def ctc_greedy_search(model, xs_pad, xs_masks, xs_lengths=None):
    """utils/recognize.py:254-270: (hyps: list of token lists with repeats and blanks removed, scores: per-utterance
    maximum frame log-probability).  `model` is a CTCGreedySearch."""
    best, logp, hyp, hyp_len = model._search(xs_pad, xs_masks)
    lens = hyp_len.cpu().tolist()
    rows = hyp.cpu().tolist()
    return [r[:n] for r, n in zip(rows, lens)], logp.max(1).values


class CTCPrefixBeamSearch(nn.Module):
    """CTC prefix beam search net (models/decoders/decoder_factory.py:195-239): forward(xs_pad, xs_masks, xs_lengths) ->
    (encoder_out (B, T', d), encoder_mask (B, 1, T'), top-k log-probabilities (B, T', beam) float32, top-k indices (B, T', beam)
    int32) - TopK(log_softmax(ctc logits), beam_size) on ma_ctc_topk_f32.  `xs_masks` is the un-subsampled (B, 1, T) pad mask."""

    def __init__(self, backbone, beam_size, pretrained_model=False):
        super().__init__()
        if pretrained_model:
            raise NotImplementedError("wav2vec front ends are outside the built path")
        self.backbone, self.beam_size = backbone, int(beam_size)

    @torch.no_grad()
    def forward(self, xs_pad, xs_masks, xs_lengths=None):
        sub = xs_masks[:, :, :-2:2][:, :, :-2:2].contiguous()
        enc, enc_mask = self.backbone.encoder(xs_pad, sub, sub)
        b, t2, _ = enc.shape
        logits = self.backbone.ctc.logits(enc)
        logp, index = ops.ctc_topk(logits, logits.shape[1], self.beam_size)
        return enc, enc_mask, logp.view(b, t2, self.beam_size), index.view(b, t2, self.beam_size)


class AttentionRescoring(nn.Module):
    """Attention rescoring net (decoder_factory.py:242-275): forward(encoder_out (B, T', d), encoder_mask (B, 1, T'), hyps_in_pad
    (B*group, L), hyps_masks (B*group, L, L), group) -> the decoder's scores (B*group, L, V) float32 before the log_softmax, which
    ma_hyp_score_f32 takes row by row.  The B encoder outputs are not repeated (TransformerDecoder.score_hypotheses)."""

    def __init__(self, backbone, beam_size, pretrained_models=False):
        super().__init__()
        if pretrained_models:
            raise NotImplementedError("wav2vec front ends are outside the built path")
        if getattr(backbone, "decoder", None) is None:
            raise NotImplementedError("attention rescoring needs the attention decoder (model_conf.ctc_weight < 1.0)")
        self.backbone, self.beam_size = backbone, int(beam_size)

    @torch.no_grad()
    def forward(self, encoder_out, encoder_mask, hyps_in_pad, hyps_masks, group=None):
        return self.backbone.decoder.score_hypotheses(encoder_out, encoder_mask, hyps_in_pad, hyps_masks,
                                                      self.beam_size if group is None else group)


def decoder_input(hyp, hyp_len, sos, eos, L1=None):
    """The rescoring decoder's input (utils/recognize.py:370-385): add_sos_eos, pad_sequence with eos, and the (n, L1, L1) mask
    ~make_pad_mask(len + 1) & subsequent_mask.  hyp (n, >= L1 - 1) int32 tokens, hyp_len (n,) -> (hyps_in_pad (n, L1) int32,
    hyps_masks (n, L1, L1) float32).  L1 defaults to the longest hypothesis + 1 instead of the reference's max_tgt_len + 1 = 31: the
    decoder is causal and the padding is masked, so the positions that count are the same (and hypotheses of more than 30 tokens fit)."""
    lens = hyp_len.to(torch.int64).reshape(-1)
    n = lens.numel()
    if L1 is None:
        L1 = int(lens.max()) + 1 if n else 1
    pos = torch.arange(L1, device=hyp.device)
    ys = torch.full((n, L1), int(eos), dtype=torch.int32, device=hyp.device)
    ys[:, 0] = int(sos)
    if L1 > 1:
        ys[:, 1:] = torch.where(pos[None, 1:] <= lens[:, None], hyp[:, :L1 - 1].to(torch.int32), ys[:, 1:])
    valid = pos[None, :] < (lens + 1)[:, None]
    sub = torch.tril(torch.ones((L1, L1), dtype=torch.bool, device=hyp.device))
    return ys, (valid[:, None, :] & sub[None]).to(torch.float32)


def _prefix_search(model, xs_pad, xs_masks):
    enc, enc_mask, logp, index = model(xs_pad, xs_masks)
    b, t2, beam = logp.shape
    mask = enc_mask.reshape(-1).to(torch.float32).contiguous()
    hyp, hyp_len, score, n_hyp = ops.ctc_prefix_beam_search(logp.reshape(b * t2, beam), index.reshape(b * t2, beam), b, t2, beam,
                                                            mask=mask)
    return enc, enc_mask, hyp, hyp_len, score, n_hyp


def ctc_prefix_beam_search(model, xs_pad, xs_masks, beam_size, xs_lengths=None):
    """utils/recognize.py:273-336 for a batch of B >= 1 (the reference asserts B == 1): model is a CTCPrefixBeamSearch of that
    beam size -> (hyps: per utterance the list of (prefix tuple, score) best first - fewer than beam_size when fewer survive,
    encoder_out (B, T', d), encoder_mask (B, 1, T')).  Every utterance's result is what a one-utterance call gives."""
    if model.beam_size != int(beam_size):
        raise ValueError("the search net was built for beam %d, not %d" % (model.beam_size, beam_size))
    enc, enc_mask, hyp, hyp_len, score, n_hyp = _prefix_search(model, xs_pad, xs_masks)
    hyp, lens, score, n_hyp = hyp.cpu().tolist(), hyp_len.cpu().tolist(), score.cpu().tolist(), n_hyp.cpu().tolist()
    out = [[(tuple(hyp[u][p][:lens[u][p]]), score[u][p]) for p in range(n_hyp[u])] for u in range(len(n_hyp))]
    return out, enc, enc_mask


def attention_rescoring(model_ctc, model_rescore, xs_pad, xs_masks, xs_lengths, sos, eos, beam_size, ctc_weight):
    """utils/recognize.py:339-406 for a batch of B >= 1: the encoder runs once, the prefix search gives up to beam_size hypotheses
    per utterance, the decoder scores all B * beam_size of them against the B encoder outputs, and each utterance keeps the first
    hypothesis with the highest sum of decoder log-probabilities (+ eos) + ctc_weight * CTC score -> (per utterance the best prefix as
    a list of tokens, per utterance its score)."""
    if model_ctc.beam_size != int(beam_size):
        raise ValueError("the search net was built for beam %d, not %d" % (model_ctc.beam_size, beam_size))
    enc, enc_mask, hyp, hyp_len, score, n_hyp = _prefix_search(model_ctc, xs_pad, xs_masks)
    b, beam, t2 = hyp.shape
    hyp2, lens = hyp.reshape(b * beam, t2), hyp_len.reshape(-1)
    ys, masks = decoder_input(hyp2, lens, sos, eos)
    l1 = ys.shape[1]
    scores = model_rescore(enc, enc_mask, ys, masks, beam)
    v = scores.shape[2]
    _, best, best_score = ops.hyp_score(scores.reshape(b * beam * l1, v), v, b, beam, l1, hyp2, lens, eos, score.reshape(-1),
                                        ctc_weight, n_hyp)
    best, best_score = best.cpu().tolist(), best_score.cpu().tolist()
    hyp_h, lens_h = hyp.cpu(), hyp_len.cpu()
    return [hyp_h[u, best[u], :int(lens_h[u, best[u]])].tolist() for u in range(b)], best_score


class Attention(nn.Module):
    """Attention net (models/decoders/decoder_factory.py:59-192), the `full_graph` form of decode_mode `attention`: the beam search
    on the Transformer decoder with the whole loop on the device.  Where the reference repeats the encoder output beam_size times
    and re-runs the decoder on the maxlen-padded prefix at every step, `begin` runs the encoder once, computes the source
    attention's K / V once per utterance (TransformerDecoder.init_cache) and hands out a step callable that advances every beam by
    one token on the key / value cache (TransformerDecoder.step); `recognize` drives it."""

    def __init__(self, backbone, beam_size, eos, pretrained_model=False):
        super().__init__()
        if pretrained_model:
            raise NotImplementedError("wav2vec front ends are outside the built path")
        if getattr(backbone, "decoder", None) is None:
            raise NotImplementedError("the attention decode mode needs the attention decoder (model_conf.ctc_weight < 1.0)")
        self.backbone, self.beam_size, self.eos = backbone, int(beam_size), int(eos)

    @torch.no_grad()
    def begin(self, xs_pad, xs_masks, xs_lengths=None):
        """xs_pad (B, T, feat), xs_masks (B, 1, T) un-subsampled -> (maxlen = the encoder's frame count, step) with
        step(tokens (B * beam,), t, parent) -> the decoder's scores (B * beam, V) float32 at position t."""
        sub = xs_masks[:, :, :-2:2][:, :, :-2:2].contiguous()
        enc, enc_mask = self.backbone.encoder(xs_pad, sub, sub)
        maxlen = enc.shape[1]
        decoder = self.backbone.decoder
        cache = decoder.init_cache(enc, enc_mask, self.beam_size, maxlen)
        return maxlen, lambda tokens, t, parent=None: decoder.step(cache, tokens, t, parent)


def recognize(model, xs_pad, xs_masks, start_token, base_index, scores, end_flag, beam_size, eos, xs_lengths=None, full_graph=True,
              chunk=8):
    """utils/recognize.py:78-251 for a batch of B >= 1 -> (best_hyps (B, maxlen - 1) int32 array, best_scores (B,) float32 array).
    `model` is an Attention (anything with beam_size and begin(xs_pad, xs_masks, xs_lengths) -> (maxlen, step callable) will do: the
    logits source of a step is a callable).  start_token (1,) = [sos], scores (beam,) = [0, -inf, ...] and end_flag (beam,) are the
    reference's initial state, tiled over the batch here; base_index is accepted for the signature (parents are global row indices).

    The encoder runs once and maxlen is its frame count.  Every step is: the callable's logits -> ma_ctc_topk_f32 (k = beam) ->
    ma_attn_beam_step_f32, whose `pred` and `parent` feed the next step; nothing is read back inside a chunk of `chunk` steps.  The
    per-utterance `done` flags are read between chunks and the loop stops when all are set (or after maxlen - 1 steps).  Steps issued
    after an utterance is done are harmless: it is frozen.

    Kept from the reference: -10000 (not -inf) on the extra branches of a finished beam, the trailing eos tokens of beams that
    finished before their utterance did, sos == eos, no length normalisation.  Not kept: the NaN of `-inf * 0` (the finished beam's
    first branch adds exactly 0), batch-wide termination (the reference goes on appending eos to a finished utterance until every
    utterance of the batch has finished; here a finished utterance is frozen, so each gets the result of a one-utterance call), and
    the host-side width T // 4 - 1 of the reference's full_graph form, which differs from the encoder's frame count only in
    trailing zeros.  full_graph=False (the host-stepped PredictNet form) is not built."""
    import numpy as np

    if not full_graph:
        raise NotImplementedError("the host-stepped form of the attention decode mode (full_graph: false) is not built; "
                                  "full_graph: true selects the device-resident search")
    beam = int(beam_size)
    if getattr(model, "beam_size", beam) != beam:
        raise ValueError("the search net was built for beam %d, not %d" % (model.beam_size, beam))
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    dev = xs_pad.device
    b = xs_pad.shape[0]
    maxlen, step = model.begin(xs_pad, xs_masks, xs_lengths)
    max_new = maxlen - 1
    i32 = torch.int32
    sc = torch.as_tensor(np.asarray(scores, np.float32).reshape(-1)).to(dev)
    ef = torch.as_tensor(np.asarray(end_flag).reshape(-1) != 0).to(dev)
    if sc.numel() != beam or ef.numel() != beam:
        raise ValueError("scores and end_flag hold one entry per beam")
    state = (sc.repeat(b).contiguous(), ef.to(i32).repeat(b).contiguous(), torch.zeros((b * beam, maxlen), dtype=i32, device=dev))
    state[2][:, 0] = int(np.asarray(start_token).reshape(-1)[0])
    if max_new < 1:
        return np.zeros((b, 0), np.int32), state[0].view(b, beam).max(1).values.cpu().numpy()
    length = torch.zeros(b, dtype=i32, device=dev)
    done = torch.zeros(b, dtype=i32, device=dev)
    tokens, parent, spare = state[2][:, 0].contiguous(), None, None
    t = 0
    with _host.pinned_stream():  # (a step is ~70 launches: torch's current stream is resolved once, not per launch)
        while t < max_new:
            for _ in range(min(int(chunk), max_new - t)):
                logits = step(tokens, t, parent)
                logp, index = ops.ctc_topk(logits, logits.shape[1], beam)
                out = ops.attn_beam_step(logp, index, state[0], state[1], state[2], length, done, eos, max_new, out=spare)
                spare = state + (parent, tokens) if parent is not None else None  # (the buffers of two steps ago are free again)
                state, parent, tokens = out[:3], out[3], out[4]
                t += 1
            if bool(done.all()):  # the one read-back of a chunk
                break
    hyp, _, best = ops.attn_beam_best(state[0], state[2], length, beam)
    return hyp.cpu().numpy(), best.cpu().numpy()
