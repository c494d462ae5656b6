"""DDRNetLoss (reference: training/losses/ddrnet_loss.py): OhemCELoss on every output of the network (main head, auxiliary head), summed with
per-output weights.  forward -> (total, stacked detached [main, aux..., total]) for the Trainer's logging."""
from typing import List, Union

import torch

from ...common.registry import register_loss
from .ohem_ce_loss import OhemCELoss


@register_loss(name="DDRNetLoss")
class DDRNetLoss(OhemCELoss):
    def __init__(self, threshold: float = 0.7, ohem_percentage: float = 0.1, weights: List[float] = (1.0, 0.4), ignore_label: int = 255,
                 num_pixels_exclude_ignored: bool = False):
        super().__init__(threshold=threshold, mining_percent=ohem_percentage, ignore_lb=ignore_label, num_pixels_exclude_ignored=num_pixels_exclude_ignored)
        self.weights = list(weights)

    def forward(self, predictions_list: Union[list, tuple, torch.Tensor], targets: torch.Tensor):
        if isinstance(predictions_list, torch.Tensor):
            predictions_list = (predictions_list,)
        if len(predictions_list) != len(self.weights):
            raise ValueError(f"num of prediction must be the same as num of loss weights: {len(predictions_list)} predictions, {len(self.weights)} weights")
        unweighted = [super(DDRNetLoss, self).forward(p, targets) for p in predictions_list]
        total = sum(u * w for u, w in zip(unweighted, self.weights))
        return total, torch.stack(unweighted + [total], dim=0).detach()

    @property
    def component_names(self):
        return ["main_loss", "aux_loss1", "loss"]
