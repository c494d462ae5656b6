"""BCEDiceLoss (reference: training/losses/bce_dice_loss.py): loss_weights[0] * mean BCE-with-logits(input, target) + loss_weights[1] *
BinaryDiceLoss(apply_sigmoid=logits)(input, target) on an [N, 1, H, W] map against a binary [N, H, W] target.  The BCE term always reads the
input as logits, as the reference's does.  Both terms come from ONE moment pass over the map and ONE gradient pass (csrc/seg_struct.h)."""
from typing import List

from torch import nn

from ...common.registry import register_loss
from .structure_loss import structure_loss


@register_loss(name="BCEDiceLoss")
class BCEDiceLoss(nn.Module):
    def __init__(self, loss_weights: List[float] = (0.5, 0.5), logits: bool = True):
        super().__init__()
        self.loss_weights, self.logits = list(loss_weights), logits

    def forward(self, input, target):
        if input.dim() != 4 or input.size(1) != 1:
            raise ValueError(f"BCEDiceLoss takes an [N, 1, H, W] map; got {tuple(input.shape)}")
        return structure_loss(input, target, act="sigmoid" if self.logits else "identity", bce_weight=self.loss_weights[0], dice_weight=self.loss_weights[1])
