"""Equal error rate: mirror of mindaudio/metric/eer.py (compute_fa_miss, get_eer, get_eer_from_scores) and of `EER` in
examples/ECAPA-TDNN/speaker_verification_cosine.py.  Host code, float64.

`compute_fa_miss` restates sklearn.metrics.roc_curve (sklearn is not a dependency of this package) with its defaults: scores sorted
descending by a stable sort, one point per distinct score, `drop_intermediate=True` (interior points where neither the false- nor
the true-positive count bends are dropped), a leading (0, 0) point with threshold `inf`.  `get_eer` calls scipy's interp1d and
brentq exactly as the reference does.

Quirks of the reference that are reproduced, not repaired (the reversed P_fa handed to interp1d holds repeated x values, so which
points survive drop_intermediate decides the answer):
  * perfectly separable scores give (0.5, inf), not 0;
  * all-equal scores give (0.5, inf);
  * one positive among 20 negatives can give an "EER" above 0.5 and a threshold interpolated towards inf;
  * labels without a positive or without a negative give NaN rates (sklearn warns) and interp1d / brentq raise ValueError.

`EER(pos, neg)` follows the example's rule - thresholds are the unique scores plus their midpoints, FRR = share of positives <=
threshold, FAR = share of negatives > threshold, first index of the minimal |FAR - FRR|, mean of the two - by sorting and
searchsorted instead of the reference's thresholds x trials boolean matrix (several GB on VoxCeleb1-O).
"""
import warnings

import numpy as np

__all__ = ["compute_fa_miss", "get_eer", "get_eer_from_scores", "EER"]


def _roc_curve(labels, scores, pos_label):
    y_true = np.ravel(np.asarray(labels))
    y_score = np.ravel(np.asarray(scores))
    if y_true.shape[0] != y_score.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (y_true.shape[0], y_score.shape[0]))
    if y_score.size == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required.")
    if not np.all(np.isfinite(y_score.astype(np.float64))):
        raise ValueError("Input contains NaN or infinity.")
    y_true = y_true == pos_label
    desc = np.argsort(y_score, kind="mergesort")[::-1]
    y_score = y_score[desc]
    y_true = y_true[desc]
    distinct = np.where(np.diff(y_score))[0]
    idx = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    thresholds = y_score[idx]
    if len(fps) > 2:  # drop_intermediate=True
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps = np.r_[0, tps]
    fps = np.r_[0, fps]
    thresholds = np.r_[np.inf, thresholds]
    if fps[-1] <= 0:
        warnings.warn("No negative samples in y_true, false positive value should be meaningless")
        fpr = np.repeat(np.nan, fps.shape)
    else:
        fpr = fps / fps[-1]
    if tps[-1] <= 0:
        warnings.warn("No positive samples in y_true, true positive value should be meaningless")
        tpr = np.repeat(np.nan, tps.shape)
    else:
        tpr = tps / tps[-1]
    return fpr, tpr, thresholds


def compute_fa_miss(scores, labels, pos_label=1, return_thresholds=True):
    """Returns P_fa, P_miss, [thresholds]"""
    fpr, tpr, thresholds = _roc_curve(labels, scores, pos_label)
    P_fa = fpr[::-1]
    P_miss = 1.0 - tpr[::-1]
    thresholds = thresholds[::-1]
    if return_thresholds:
        return P_fa, P_miss, thresholds
    return P_fa, P_miss


def get_eer(P_fa, P_miss, thresholds=None):
    """Compute EER given false alarm and miss probabilities"""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq

    eer = brentq(lambda x: x - interp1d(P_fa, P_miss)(x), 0.0, 1.0)
    eer = float(eer)
    if thresholds is None:
        return eer
    thresh_eer = interp1d(P_fa, thresholds)(eer)
    thresh_eer = float(thresh_eer)
    return eer, thresh_eer


def get_eer_from_scores(scores, labels, pos_label=1):
    """Compute EER given scores and labels"""
    P_fa, P_miss, thresholds = compute_fa_miss(scores, labels, pos_label, return_thresholds=True)
    eer, thresh_eer = get_eer(P_fa, P_miss, thresholds)
    return eer, thresh_eer


def EER(pos_arr, neg_arr):
    """The example's EER over positive and negative score arrays (see the module docstring), in O(n log n) time and O(n) memory."""
    pos = np.sort(np.asarray(pos_arr, dtype=np.float64).ravel())
    neg = np.sort(np.asarray(neg_arr, dtype=np.float64).ravel())
    thresholds = np.unique(np.concatenate((pos, neg)))
    interm = (thresholds[0:-1] + thresholds[1:]) / 2
    thresholds = np.sort(np.concatenate((thresholds, interm)))
    FRR = np.searchsorted(pos, thresholds, side="right") / pos.shape[0]
    FAR = (neg.shape[0] - np.searchsorted(neg, thresholds, side="right")) / neg.shape[0]
    min_index = np.argmin(np.absolute(FAR - FRR))
    return (FAR[min_index] + FRR[min_index]) / 2
