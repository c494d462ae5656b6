"""OhemCELoss (reference: training/losses/ohem_ce_loss.py:7-74): online hard example mining over the per-pixel cross-entropy of an
[N, C, H, W] map.  With more than num_mining = int(mining_percent * num_pixels) losses above -log(threshold) the loss is the mean of those,
otherwise the mean of the num_mining largest.  The reference sorts the N*H*W losses and reads loss[num_mining] back; here the per-pixel losses,
the branch, the selection by rank and the gradient are kernels.seg_ohem_ce (csrc/seg_ohem.h) and nothing is read back.
Two deviations, both forced by that: bit-equal losses across the rank boundary share the remaining weight equally (torch.sort keeps an
unspecified subset: the loss value is the same), and a map whose pixels are all ignored gives the 0-dim scalar 0, not a [1] tensor (a shape
cannot depend on device data)."""
import torch
from torch import nn

from ... import kernels as K
from ...common.registry import register_loss


class _OhemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, cfg):
        loss, dlogits = K.seg_ohem_ce(logits, labels, *cfg)
        ctx.save_for_backward(dlogits)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return K.scale_by_device_scalar(dlogits, g.reshape(1).contiguous()), None, None


@register_loss(name="OhemCELoss")
class OhemCELoss(nn.Module):
    def __init__(self, threshold: float, mining_percent: float = 0.1, ignore_lb: int = -100, num_pixels_exclude_ignored: bool = True):
        super().__init__()
        if mining_percent < 0 or mining_percent > 1:
            raise ValueError(f"mining percent must be in range (0, 1), got {mining_percent}")
        self.threshold = float(threshold)
        self.thresh = -torch.log(torch.tensor(threshold, dtype=torch.float))
        self.mining_percent = mining_percent
        self.ignore_lb = -100 if ignore_lb is None or ignore_lb < 0 else int(ignore_lb)
        self.num_pixels_exclude_ignored = bool(num_pixels_exclude_ignored)

    def forward(self, logits, labels):
        if logits.dim() != 4 or labels.dim() != 3 or labels.is_floating_point():
            raise ValueError(f"OhemCELoss takes logits [N, C, H, W] and integer labels [N, H, W]; got {tuple(logits.shape)} and {labels.dtype} {tuple(labels.shape)}")
        cfg = (self.threshold, self.mining_percent, self.ignore_lb, self.num_pixels_exclude_ignored)
        return _OhemFn.apply(logits, labels.to(logits.device), cfg)
