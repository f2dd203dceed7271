"""Convtasnet_Loss (mindaudio/loss/separation_loss.py:140-264) and Separation_Loss (:13-130, TasNet's): SI-SNR with
permutation-invariant training, evaluation side (no backward).  The pairwise SI-SNR table is a float64 device kernel
(ops.si_snr_pairwise)."""
from .. import ops

__all__ = ["Convtasnet_Loss", "Separation_Loss"]

EPS = 1e-8


class Convtasnet_Loss:
    """__call__(source (B, C, T), estimate_source (B, C, T), source_lengths (B)) -> (loss, max_snr (B, 1), estimate_source,
    reorder_estimate_source), C from 1 to 4.

    Both signals are zero-meaned over the valid samples (sum / length), the pairwise SI-SNR [b, i_est, j_target] carries EPS = 1e-8
    where separation_loss.py:205-216 puts it, the best of itertools.permutations(range(C)) wins (the first on a tie),
    max_snr = best / C, loss = -mean(max_snr), reordered[b, j] = estimate[b, perm[j]].

    Two departures from the reference, neither visible in its example:
      * the padding mask follows `source_lengths` - positions at and beyond lengths[b] are masked.  The reference's `get_mask`
        hard-codes 46400 samples and ignores the lengths; with the example's 32000-sample segments both give an all-ones mask;
      * the caller's `estimate_source` is left as it is (the reference multiplies it by the mask in place)."""

    def __call__(self, source, estimate_source, source_lengths):
        loss, max_snr, reordered, _, _ = ops.si_snr_pit(source, estimate_source, source_lengths)
        return loss, max_snr, estimate_source, reordered

    cal_loss = __call__


class Separation_Loss:
    """__call__(source (B, C, K, L), estimate_source (B, C, K, L), source_lengths (B), in SEGMENTS) -> (loss, max_snr (B, 1),
    estimate_source, reorder_estimate_source (B, C, K, L)): TasNet's loss, separation_loss.py:13-130, with C = 2 as there.

    K and L are flattened to T = K L; both signals are zero-meaned by sum / (L * source_lengths); the pairwise SI-SNR
    [b, i_est, j_target] carries EPS = 1e-8 where the reference puts it; of the two permutations the identity wins a tie;
    max_snr = best / 2, loss = -mean(max_snr), reordered[b, j] = estimate[b, perm[j]].  There is NO padding mask: the reference's
    `get_mask` is never called, so every one of the K L samples enters every sum, whatever the length says.

    When every length equals K - the only value examples/tasnet/data.py produces - this is ops.si_snr_pit on the flattened view with
    full lengths (the float64 device kernel).  Other lengths reproduce the reference's unmasked arithmetic in float64 tensor ops (not
    a hot path).  The caller's `estimate_source` is returned as it is."""

    def __call__(self, source, estimate_source, source_lengths):
        import torch

        if source.dim() != 4 or source.shape != estimate_source.shape:
            raise ValueError("source and estimate_source must both be (B, C, K, L)")
        B, C, K, L = source.shape
        if C != 2:
            raise NotImplementedError("Separation_Loss is the reference's two-speaker loss (its permutation table is fixed at C = 2)")
        lens = torch.as_tensor(source_lengths).reshape(-1).to(torch.int64).cpu()
        if lens.numel() != B:
            raise ValueError("source_lengths must hold one length per utterance")
        if bool((lens == K).all()):
            flat_s, flat_e = source.reshape(B, C, K * L).contiguous(), estimate_source.reshape(B, C, K * L).contiguous()
            loss, max_snr, reordered, _, _ = ops.si_snr_pit(flat_s, flat_e, torch.full((B,), K * L, dtype=torch.int64))
            return loss, max_snr, estimate_source, reordered.reshape(B, C, K, L)
        dev = estimate_source.device
        s, e = source.to(dev, torch.float64).reshape(B, C, K * L), estimate_source.to(torch.float64).reshape(B, C, K * L)
        n = (L * lens).to(dev, torch.float64).reshape(B, 1, 1)
        s, e = s - s.sum(2, keepdim=True) / n, e - e.sum(2, keepdim=True) / n
        tgt, est = s[:, None, :, :], e[:, :, None, :]                       # (B, 1, C, T), (B, C, 1, T)
        proj = (est * tgt).sum(3, keepdim=True) * tgt / ((tgt ** 2).sum(3, keepdim=True) + EPS)
        pair = (proj ** 2).sum(3) / (((est - proj) ** 2).sum(3) + EPS)
        pair = 10.0 * torch.log10(pair + EPS)                               # (B, C_est, C_target)
        snr_set = torch.stack([pair[:, 0, 0] + pair[:, 1, 1], pair[:, 0, 1] + pair[:, 1, 0]], dim=1)
        swap = snr_set[:, 1] > snr_set[:, 0]                                # (Argmax returns the first index on a tie)
        max_snr = (torch.where(swap, snr_set[:, 1], snr_set[:, 0]) / C).to(torch.float32).reshape(B, 1)
        reordered = torch.where(swap[:, None, None, None], estimate_source.flip(1), estimate_source)
        return -max_snr.mean(), max_snr, estimate_source, reordered

    cal_loss = __call__
