"""Convtasnet_Loss of mindaudio/loss/separation_loss.py:140-264: SI-SNR with permutation-invariant training, evaluation side (no
backward).  The pairwise SI-SNR table is a float64 device kernel (ops.si_snr_pairwise)."""
from .. import ops

__all__ = ["Convtasnet_Loss"]


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
