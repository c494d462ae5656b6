"""PixelAccuracy and IoU (reference: training/metrics/segmentation_metrics.py:197-248, :281-331) on integer confusion counts.

Each `update` is ONE kernels.seg_confusion launch on the model's NCHW logits - the arg-max over the class planes, the label and the count
happen in that launch, nothing else runs on the device and nothing is read back; `compute` reads the small int64 matrix
counts[bins + 1][bins] (row = label, column = prediction, last row = labels outside [0, bins)) - the only host read.

IoU as DEFINED here (a restatement of what the reference inherits from torchmetrics 0.8's JaccardIndex, not checked against
that package): every pixel is counted, also one labelled `ignore_index`; with `ignore_index` in [0, num_classes) its ROW is zeroed; per class
intersection = diagonal, union = row sum + column sum - intersection, score = intersection / union, 0.0 where the union is 0; the score of
class `ignore_index` is dropped; the rest are averaged ("elementwise_mean") or summed ("sum").  Labels outside [0, num_classes) take no part.

Not built (NotImplementedError): a custom `metrics_args_prep_fn` (the launch IS the arg-max pre-processing), `dist_sync_on_step=True`, a list
of ignored indices / `threshold` / reduction "none" for IoU, more than 4 ignored labels for PixelAccuracy; Dice and the binary metrics.
"""
from typing import Iterable

import numpy as np
import torch

from ... import kernels as K
from ...common.registry import register_metric


class _ConfusionMetric:
    greater_is_better = True

    def __init__(self, dist_sync_on_step, metrics_args_prep_fn):
        if metrics_args_prep_fn is not None:
            raise NotImplementedError(f"{type(self).__name__} on the HIP path: the arg-max over the class planes is part of the counting launch (no metrics_args_prep_fn)")
        if dist_sync_on_step:
            raise NotImplementedError(f"{type(self).__name__} on the HIP path: dist_sync_on_step=True is not built")
        self.counts = None

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()

    def _count(self, preds, target, bins, ignore_labels):
        if isinstance(preds, (list, tuple)):
            preds = preds[0]
        bins = max(bins, int(preds.shape[1]))
        if self.counts is None or self.counts.shape[1] != bins or self.counts.device != preds.device:
            self.counts = None  # (first batch, or a model with more classes than the bins seen so far)
        self.counts = K.seg_confusion(preds.detach(), target.to(preds.device), bins, ignore_labels, counts=self.counts)

    def _matrix(self):
        return None if self.counts is None else self.counts.cpu().numpy()


@register_metric("PixelAccuracy")
class PixelAccuracy(_ConfusionMetric):
    def __init__(self, ignore_label=-100, dist_sync_on_step=False, metrics_args_prep_fn=None):
        super().__init__(dist_sync_on_step, metrics_args_prep_fn)
        self.ignore_label = ignore_label
        self._ignored = [int(v) for v in ignore_label] if isinstance(ignore_label, Iterable) else [int(ignore_label)]
        if len(self._ignored) > 4:
            raise NotImplementedError(f"PixelAccuracy on the HIP path: at most 4 ignored labels, got {len(self._ignored)}")

    def update(self, preds, target):
        self._count(preds, target, 0, self._ignored)

    def compute(self):
        m = self._matrix()
        correct, labelled = (np.int64(0), np.int64(0)) if m is None else (np.trace(m[:-1]), m.sum())
        return np.float64(1.0) * correct / (np.spacing(1, dtype=np.float64) + labelled)


@register_metric("IoU")
class IoU(_ConfusionMetric):
    def __init__(self, num_classes, dist_sync_on_step=False, ignore_index=None, reduction="elementwise_mean", threshold=0.5, metrics_args_prep_fn=None):
        if num_classes <= 1:
            raise ValueError("IoU class only for multi-class usage! (BinaryIOU is not built on the HIP path)")
        if isinstance(ignore_index, Iterable):
            raise NotImplementedError("IoU on the HIP path: a single ignore_index (a list of ignored indices is not built)")
        if threshold != 0.5:
            raise NotImplementedError("IoU on the HIP path: class-index predictions from the arg-max (no probability threshold)")
        if reduction not in ("elementwise_mean", "sum"):
            raise NotImplementedError(f"IoU on the HIP path: reduction 'elementwise_mean' or 'sum', got {reduction!r}")
        super().__init__(dist_sync_on_step, metrics_args_prep_fn)
        self.num_classes, self.ignore_index, self.reduction = int(num_classes), ignore_index, reduction

    def update(self, preds, target):
        self._count(preds, target, self.num_classes, ())

    def compute(self):
        m = self._matrix()
        n = self.num_classes
        m = np.zeros((n, n), dtype=np.int64) if m is None else m[:n, :n].copy()  # (more bins than num_classes: a wider model; its extra classes take no part)
        drop = self.ignore_index is not None and 0 <= self.ignore_index < n
        if drop:
            m[self.ignore_index] = 0
        inter = np.diag(m).astype(np.float64)
        union = m.sum(0).astype(np.float64) + m.sum(1).astype(np.float64) - inter
        score = np.divide(inter, union, out=np.zeros(n, dtype=np.float64), where=union > 0)
        if drop:
            score = np.delete(score, self.ignore_index)
        return np.float64(score.mean() if self.reduction == "elementwise_mean" else score.sum())
