"""ShelfNetOHEMLoss (reference: training/losses/shelfnet_ohem_loss.py): OhemCELoss on each of the network's three outputs, summed unweighted."""
import torch

from ...common.registry import register_loss
from .ohem_ce_loss import OhemCELoss


@register_loss(name="ShelfNetOHEMLoss", deprecated_name="shelfnet_ohem_loss")
class ShelfNetOHEMLoss(OhemCELoss):
    def __init__(self, threshold: float = 0.7, mining_percent: float = 1e-4, ignore_lb: int = 255):
        super().__init__(threshold=threshold, mining_percent=mining_percent, ignore_lb=ignore_lb)

    def forward(self, predictions_list: list, targets):
        losses = [super(ShelfNetOHEMLoss, self).forward(p, targets) for p in predictions_list]
        total = sum(losses)
        return total, torch.stack(losses + [total], dim=0).detach()

    @property
    def component_names(self):
        return ["Loss1/4", "Loss1/8", "Loss1/16", "Loss"]
