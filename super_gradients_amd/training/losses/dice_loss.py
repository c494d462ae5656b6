"""DiceLoss, BinaryDiceLoss, GeneralizedDiceLoss (reference: training/losses/dice_loss.py): loss_g = 1 - (2 I_g + smooth) / (D_g + eps + smooth) with
I = sum t p and D = sum t + sum p over the valid pixels; the generalized form weighs both by 1 / (sum t)^2.  The kernels are structure_loss.py's."""
from .structure_loss import AbstarctSegmentationStructureLoss


class DiceLoss(AbstarctSegmentationStructureLoss):
    iou = False


class BinaryDiceLoss(DiceLoss):
    """One class: predictions [N, 1, H, W] against a binary map [N, 1, H, W] or [N, H, W]."""

    def __init__(self, apply_sigmoid: bool = True, smooth: float = 1.0, eps: float = 1e-5):
        super().__init__(apply_softmax=False, ignore_index=None, smooth=smooth, eps=eps, reduce_over_batches=False)
        self.apply_sigmoid = apply_sigmoid


class GeneralizedDiceLoss(DiceLoss):
    def __init__(self, apply_softmax: bool = True, ignore_index: int = None, smooth: float = 0.0, eps: float = 1e-17, reduce_over_batches: bool = False,
                 reduction: str = "mean"):
        super().__init__(apply_softmax=apply_softmax, ignore_index=ignore_index, smooth=smooth, eps=eps, reduce_over_batches=reduce_over_batches,
                         generalized_metric=True, weight=None, reduction=reduction)
