"""mindaudio.loss on MI355X: AdditiveAngularMargin (mindaudio/loss/AdditiveAngularMargin.py), an elementwise device op built from
the same device functions as the fused head (ops.aam_softmax_loss, which a training step should call instead)."""
import math

from .. import ops
from .separation_loss import Convtasnet_Loss, Separation_Loss

__all__ = ["AdditiveAngularMargin", "Convtasnet_Loss", "Separation_Loss"]


class AdditiveAngularMargin:
    """AAM of the reference: __call__(outputs, targets) with `outputs` the cosines and `targets` their one-hot labels (float32 device
    tensors of one shape) -> scale * (targets * phi + (1 - targets) * outputs), phi = cos(theta + margin) where the reference keeps
    it.  Where rounding pushed |cosine| past 1 the reference's sqrt yields NaN; here the sine is sqrt(max(1 - cosine^2, 0))."""

    def __init__(self, margin=0.0, scale=1.0, easy_margin=False):
        self.margin = margin
        self.scale = scale
        self.easy_margin = easy_margin
        self.cos_m = math.cos(self.margin)
        self.sin_m = math.sin(self.margin)
        self.th = math.cos(math.pi - self.margin)
        self.mm = math.sin(math.pi - self.margin) * self.margin

    def __call__(self, outputs, targets):
        return ops.aam_margin(outputs, targets, self.margin, self.scale, self.easy_margin)
