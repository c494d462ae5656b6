"""What every classifier family shares around its own blocks: the input check, the pooled linear head with its optional dropout, head
replacement and the fine-tuning dictionary.  The detectors stay on SgxNetwork.

A family writes its blocks, `_fwd` / `_bwd` with its own bucket walk, `gradient_buckets()`, `get_input_channels()`, and names its head:
    _head_path     dotted path of the LinearLayer that replace_head() swaps ("linear", "classifier.1", "net.head.fc")
    _finetune_key  the parameter-name prefix get_finetune_lr_dict() trains (the reference's per-family key; not always the head path)
There is deliberately no generic driver or bucket walker here.
"""
from typing import Dict

import torch

from .. import kernels as K
from ..training.utils.utils import get_param
from .engine import SgxNetwork
from .layers import LinearLayer


def num_classes_of(arch_params, num_classes):
    """The reference's `num_classes or arch_params.num_classes`.  Its registered classes default num_classes to 1000, which hides
    arch_params.num_classes - the only place models.get() puts the caller's value; here the default is None, as in the other families."""
    return num_classes or get_param(arch_params, "num_classes")


def dropout_seed(training: bool, p: float):
    """The Philox seed of one dropout mask, drawn from torch's default generator (torch.manual_seed repeats a step) - or None, with
    nothing drawn, where no mask is applied (eval mode, p == 0).  The backward regenerates the mask from the same seed."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if (training and p > 0) else None


class SgxClassifier(SgxNetwork):
    _head_path = None
    _finetune_key = None

    def _input_nhwc(self, x):
        cin = self.get_input_channels()
        if x.dim() != 4 or x.shape[1] != cin:
            raise ValueError(f"expected an NCHW batch with {cin} channels, got {tuple(x.shape)}")
        return K.input_to_nhwc(x)

    # ---- global average pool -> [dropout] -> linear ---------------------------------------------------------------
    def _pool_head_fwd(self, a, head, dropout_p=0.0):
        p = float(dropout_p)
        pooled = K.avgpool_fwd(a)
        seed = dropout_seed(self.training, p)
        if seed is not None:
            pooled = K.dropout(pooled, p, seed)
        self._pool_ctx = (tuple(a.shape), seed, p)
        return head.fwd(pooled).contiguous()

    def _pool_head_bwd(self, d_logits, head):
        """-> the feature map's gradient; the caller announces the head's bucket"""
        feat_shape, seed, p = self._pool_ctx
        d = head.bwd(d_logits.contiguous()).contiguous()
        if seed is not None:
            d = K.dropout(d, p, seed, out=d)  # the same mask, regenerated
        return K.avgpool_bwd(d, feat_shape)

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def replace_head(self, new_num_classes=None, new_head=None):
        if new_num_classes is None and new_head is None:
            raise ValueError("At least one of new_num_classes, new_head must be given to replace output layer.")
        if new_head is not None:
            raise NotImplementedError("replace_head(new_head=...) is not on the HIP path; pass new_num_classes")
        if self._materialized:
            raise RuntimeError("replace_head must be called before the model is materialized in HBM")
        self._new_head(new_num_classes)

    def _new_head(self, new_num_classes):
        """A fresh LinearLayer of the old one's input width at `_head_path`; families that do more (re-initialise, rebuild a head
        module, track num_classes) override this."""
        owner, _, name = self._head_path.rpartition(".")
        owner = self.get_submodule(owner)
        setattr(owner, name, LinearLayer(getattr(owner, name).in_features, new_num_classes))

    def get_finetune_lr_dict(self, lr: float) -> Dict[str, float]:
        return {self._finetune_key: lr, "default": 0}
