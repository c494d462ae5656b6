"""The region ("structure") losses' shared base (reference: training/losses/structure_loss.py): Dice and IoU between p = act(predict) and a
one-hot or dense target, per class over the batch or per image over its classes.  The reference chains full-size ATen temporaries (softmax,
one-hot, product, sum, mask) and autograd reverses them; here forward is kernels.seg_struct_fwd (one pass over the map and a finalize step) and
backward is kernels.seg_struct_bwd (one pass that writes the gradient once) - csrc/seg_struct.h, DESIGN.md 28.
Deviations: a label whose one-hot channel falls outside the C channels masks its pixel out (the reference's F.one_hot raises; seg_ce's
convention here), and softmax against a dense target is not built (NotImplementedError)."""
from typing import Optional

import torch
from torch import nn

from ... import kernels as K


class _StructFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predict, target, cfg):
        loss, (x, t, flags, ignore, coef) = K.seg_struct_fwd(predict, target, **cfg)
        ctx.save_for_backward(x, t, coef)
        ctx.launch = (flags, ignore)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        x, t, coef = ctx.saved_tensors
        return K.seg_struct_bwd((x, t, *ctx.launch, coef), g), None, None


def structure_loss(predict, target, **cfg):
    """kernels.seg_struct_fwd / seg_struct_bwd as one differentiable call; the target forms are the reference's forward's."""
    if predict.dim() != 4:
        raise ValueError(f"structure losses take predictions [N, C, H, W]; got {tuple(predict.shape)}")
    if target.size() != predict.size():
        if target.dim() != 3 or tuple(target.shape) != (predict.shape[0],) + tuple(predict.shape[2:]):
            raise AssertionError(f"Mismatch of target shape: {target.size()} and prediction shape: {predict.size()}, target must be [NxWxH] tensor for "
                                 f"to_one_hot conversion or to have the same num of channels like prediction tensor")
        if predict.size(1) == 1 and cfg.get("ignore_index") is None:  # one class prediction task: the target is the dense plane
            target = target.unsqueeze(1)
        elif target.is_floating_point():
            raise ValueError("a [N, H, W] target of a multi-class prediction holds integer class labels")
    return _StructFn.apply(predict, target, cfg)


class AbstarctSegmentationStructureLoss(nn.Module):
    """`iou` is the subclass's metric.  Constructor arguments and defaults are the reference's."""
    iou = False

    def __init__(self, apply_softmax: bool = True, ignore_index: int = None, smooth: float = 1.0, eps: float = 1e-5, reduce_over_batches: bool = False,
                 generalized_metric: bool = False, weight: Optional[torch.Tensor] = None, reduction: str = "mean"):
        super().__init__()
        reduction = getattr(reduction, "value", reduction)
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"Reduction mode is not supported, expected options are ['mean', 'sum', 'none'], found {reduction}")
        if generalized_metric and weight is not None:
            raise ValueError("Cannot use structured Loss with weight classes and generalized normalization")
        if reduce_over_batches and weight is not None:
            raise ValueError("class weights need the classes as groups: reduce_over_batches=False")
        self.ignore_index, self.apply_softmax, self.eps, self.smooth = ignore_index, apply_softmax, eps, smooth
        self.reduce_over_batches, self.generalized_metric, self.reduction = reduce_over_batches, generalized_metric, reduction
        self.weight = None if weight is None else torch.as_tensor(weight, dtype=torch.float32)
        self.apply_sigmoid = False

    def forward(self, predict, target):
        if target.size() == predict.size() and self.ignore_index is not None:
            raise ValueError("a dense target cannot be combined with ignore_index (the reference's mask does not broadcast there)")
        act = "softmax" if self.apply_softmax else ("sigmoid" if self.apply_sigmoid else "identity")
        return structure_loss(predict, target, act=act, iou=self.iou, reduce_over_batches=self.reduce_over_batches, generalized=self.generalized_metric,
                              reduction=self.reduction, ignore_index=self.ignore_index, smooth=self.smooth, eps=self.eps, weight=self.weight)
