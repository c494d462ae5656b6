"""MobileNetV3 classifiers on the HIP kernels.

Reference: training/models/classification_models/mobilenetv3.py - _make_divisible (:18-31), h_sigmoid / h_swish (:34-49), SELayer (:52-67),
InvertedResidual (:78-118, both layouts), MobileNetV3 (:121-182), mobilenetv3_large / _small / _custom (:185-252).  Same constructor
arguments, cfg tables, `_make_divisible` rule, last-channel rule (1280 / 1024, scaled only for width_mult > 1), initial weight distributions
and state_dict keys (features.0.{0,1}.*, features.{i}.conv.{j}.* incl. ...conv.{5|3}.fc.{0,2}.*, conv.{0,1}.*, classifier.{0,3}.*), so
checkpoints interchange both ways.

Kernel sequence (training), per inverted residual (DESIGN.md 16 counts the passes):
  expanded layout (inp != hidden):  1x1 conv -> bn_finalize -> affine + act sweep; depthwise 3x3 / 5x5 (statistics in its launch) ->
    bn_finalize -> [no SE: affine + act sweep | SE: image_colsum of the raw convolution output -> the means through scale / shift on [N,C] ->
    Linear, ReLU, Linear -> ONE sweep act(gate * (scale * t + shift))]; 1x1 projection -> bn_finalize -> affine sweep (+ the residual).
  inp == hidden layout:  depthwise -> bn_finalize -> affine + act sweep -> [SE: image_colsum -> fc -> channel_gate] -> projection as above.
Backward with SE between BatchNorm and activation: one reduction for d(pre), the fc backward on [N,C], one sweep that writes dz and the
BatchNorm backward's reduce rows, then bn_bwd_finalize + bn_bwd_apply - no separate reduce sweep.  Classifier: Linear -> hard-swish sweep ->
dropout (Philox mask regenerated in the backward, seed drawn from torch's default generator) -> Linear.  Eval after
prep_model_for_conversion(): every conv + BatchNorm folds; a depthwise layer is act(dwconv + bias) in one launch, with SE dwconv + bias
followed by the gate sweep without scale / shift.

Not built (each raises NotImplementedError): widths that are not multiples of 4; kernel sizes other than 3 / 5; replace_head(new_head=...).
"""
import torch

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNSeq, ConvBNView
from ....modules.classifier import SgxClassifier, dropout_seed, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import (BatchNorm, ConvLayer, DepthwiseConvLayer, Dropout, LinearLayer, Numbered, init_normal_fan_out,
                                 need_mult4)
from ....modules.se_blocks import SELayer, _make_divisible
from ...utils.utils import get_param

LARGE_CFGS = [
    # k, t, c, SE, HS, s
    [3, 1, 16, 0, 0, 1], [3, 4, 24, 0, 0, 2], [3, 3, 24, 0, 0, 1], [5, 3, 40, 1, 0, 2], [5, 3, 40, 1, 0, 1], [5, 3, 40, 1, 0, 1],
    [3, 6, 80, 0, 1, 2], [3, 2.5, 80, 0, 1, 1], [3, 2.3, 80, 0, 1, 1], [3, 2.3, 80, 0, 1, 1], [3, 6, 112, 1, 1, 1], [3, 6, 112, 1, 1, 1],
    [5, 6, 160, 1, 1, 2], [5, 6, 160, 1, 1, 1], [5, 6, 160, 1, 1, 1],
]
SMALL_CFGS = [
    [3, 1, 16, 1, 0, 2], [3, 4.5, 24, 0, 0, 2], [3, 3.67, 24, 0, 0, 1], [5, 4, 40, 1, 1, 2], [5, 6, 40, 1, 1, 1], [5, 6, 40, 1, 1, 1],
    [5, 3, 48, 1, 1, 1], [5, 3, 48, 1, 1, 1], [5, 6, 96, 1, 1, 2], [5, 6, 96, 1, 1, 1], [5, 6, 96, 1, 1, 1],
]


class InvertedResidual(SgxBlock):
    """Reference InvertedResidual, both layouts: inp == hidden_dim: dw, BN, act, SE, 1x1, BN (keys conv.{0,1,3,4,5}); otherwise 1x1, BN, act,
    dw, BN, SE, act, 1x1, BN (keys conv.{0,1,3,4,5,7,8})."""

    def __init__(self, inp, hidden_dim, oup, kernel_size, stride, use_se, use_hs):
        super().__init__()
        assert stride in (1, 2)
        if kernel_size not in (3, 5):
            raise NotImplementedError(f"MobileNetV3 on the HIP path: depthwise kernel size 3 or 5, got {kernel_size}")
        need_mult4("MobileNetV3", "block input width", inp)
        need_mult4("MobileNetV3", "hidden width", hidden_dim)
        need_mult4("MobileNetV3", "block output width", oup)
        self.stride = stride
        self.identity = stride == 1 and inp == oup
        act = "hswish" if use_hs else "relu"
        se = SELayer(hidden_dim) if use_se else None
        dw = DepthwiseConvLayer(hidden_dim, stride, kernel_size)
        if inp == hidden_dim:
            layers = {"0": dw, "1": BatchNorm(hidden_dim), "4": ConvLayer(hidden_dim, oup, 1, 1, 0), "5": BatchNorm(oup)}
            if se is not None:
                layers["3"] = se
            self.conv = Numbered(**{k: layers[k] for k in sorted(layers)})
            self.pw = None
            self.dw = ConvBNView(layers["0"], layers["1"], act)
            self.se_after = se
            self.pwl = ConvBNView(layers["4"], layers["5"], None)
        else:
            layers = {"0": ConvLayer(inp, hidden_dim, 1, 1, 0), "1": BatchNorm(hidden_dim), "3": dw, "4": BatchNorm(hidden_dim),
                      "7": ConvLayer(hidden_dim, oup, 1, 1, 0), "8": BatchNorm(oup)}
            if se is not None:
                layers["5"] = se
            self.conv = Numbered(**{k: layers[k] for k in sorted(layers)})
            self.pw = ConvBNView(layers["0"], layers["1"], act)
            self.dw = ConvBNView(layers["3"], layers["4"], act, gate=se)
            self.se_after = None
            self.pwl = ConvBNView(layers["7"], layers["8"], None)

    def on_materialize(self):
        pass

    def __setattr__(self, name, value):
        if name == "se_after":  # (registered under conv.3 already: kept out of the module registry here)
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    def fwd(self, x, out=None):
        a = self.pw.fwd(x) if self.pw is not None else x
        a = self.dw.fwd(a)
        if self.se_after is not None:
            a = self.se_after.fwd(a)
        return self.pwl.fwd(a, out=out, residual=x if self.identity else None)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        if addend is not None:
            raise NotImplementedError("InvertedResidual.bwd: no addend (the residual uses the first data gradient's)")
        res = dy if self.identity else None  # d(x + conv(x)) = dy + d conv: dy joins the block's first data gradient
        d = self.pwl.bwd(dy)
        if self.se_after is not None:
            d = self.se_after.bwd(d)
        first = self.pw if self.pw is not None else self.dw
        if first is not self.dw:
            d = self.dw.bwd(d)
        return first.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=res, need_dx=need_dx)


class MobileNetV3(SgxClassifier):
    _head_path, _finetune_key = "classifier.3", "classifier"

    def __init__(self, cfgs, mode, num_classes=1000, width_mult=1.0, in_channels: int = 3):
        super().__init__()
        self.cfgs = cfgs
        assert mode in ["large", "small"]
        curr = _make_divisible(16 * width_mult, 8)
        feats = [ConvBNSeq(in_channels, curr, 3, stride=2, padding=1, activation_type="hswish")]
        exp_size = curr
        for k, t, c, use_se, use_hs, s in self.cfgs:
            oup = _make_divisible(c * width_mult, 8)
            exp_size = _make_divisible(curr * t, 8)
            feats.append(InvertedResidual(curr, exp_size, oup, k, s, use_se, use_hs))
            curr = oup
        need_mult4("MobileNetV3", "the last block's width", curr)
        self.features = Numbered(feats)
        self.conv = ConvBNSeq(curr, exp_size, 1, stride=1, padding=0, activation_type="hswish")
        last = {"large": 1280, "small": 1024}[mode]
        self.last_channel = _make_divisible(last * width_mult, 8) if width_mult > 1.0 else last
        self.exp_size = exp_size
        self.classifier = Numbered(**{"0": LinearLayer(exp_size, self.last_channel), "2": Dropout(0.2), "3": LinearLayer(self.last_channel, num_classes)})
        init_normal_fan_out(self, (ConvLayer, DepthwiseConvLayer))  # (reference :161-174)

    def _fwd(self, x):
        a = self._input_nhwc(x)
        for f in self.features.blocks():
            a = f.fwd(a)
        a = self.conv.fwd(a)
        self._feat_shape = tuple(a.shape)
        pooled = K.avgpool_fwd(a)
        n = pooled.shape[0]
        cls = self.classifier._modules
        h = cls["0"].fwd(pooled).contiguous().view(n, 1, 1, self.last_channel)
        a = K.affine_act(h, act="hswish")
        p = float(cls["2"].p)
        seed = dropout_seed(self.training, p)
        self._cls = (h, seed, p) if self.training else None
        if seed is not None:
            a = K.dropout(a, p, seed)
        logits = cls["3"].fwd(a.view(n, self.last_channel))
        return (logits.contiguous(),)

    def _bwd(self, d_logits):
        cls = self.classifier._modules
        (h, seed, p), self._cls = self._cls, None
        n = h.shape[0]
        d = cls["3"].bwd(d_logits.contiguous()).contiguous().view(n, 1, 1, self.last_channel)
        if seed is not None:
            d = K.dropout(d, p, seed, out=d)  # the same mask, regenerated
        # d * hswish'(h): the gate sweep's data gradient with a unit gate (f(pre) = pre = 1) and no BatchNorm affine
        ones = torch.ones(n, self.last_channel, device=h.device)
        d = K.bn_gate_act_bwd_data(d, h, None, None, ones, "none", act="hswish", out=d)
        d = cls["0"].bwd(d.view(n, self.last_channel))
        d = K.avgpool_bwd(d.contiguous(), self._feat_shape)
        ready = self._bucket_ready
        ready("classifier.")
        d = self.conv.bwd(d)
        ready("conv.")
        feats = self.features.blocks()
        for i in range(len(feats) - 1, 0, -1):
            d = feats[i].bwd(d)
            ready(f"features.{i}.")
        feats[0].bwd(d, need_dx=False)
        ready("features.0.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return [f"features.{i}." for i in range(len(self.features.blocks()))] + ["conv.", "classifier."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.features._modules["0"]._modules["0"].in_channels


@register_model("mobilenet_v3_large")
class mobilenetv3_large(MobileNetV3):
    def __init__(self, arch_params, num_classes=None):
        super().__init__([list(r) for r in LARGE_CFGS], mode="large", num_classes=num_classes_of(arch_params, num_classes),
                         width_mult=get_param(arch_params, "width_mult", 1.0), in_channels=get_param(arch_params, "in_channels", 3))


@register_model("mobilenet_v3_small")
class mobilenetv3_small(MobileNetV3):
    def __init__(self, arch_params, num_classes=None):
        super().__init__([list(r) for r in SMALL_CFGS], mode="small", num_classes=num_classes_of(arch_params, num_classes),
                         width_mult=get_param(arch_params, "width_mult", 1.0), in_channels=get_param(arch_params, "in_channels", 3))


@register_model("mobilenet_v3_custom")
class mobilenetv3_custom(MobileNetV3):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(cfgs=get_param(arch_params, "structure"), mode=get_param(arch_params, "mode"),
                         num_classes=num_classes_of(arch_params, num_classes), width_mult=get_param(arch_params, "width_mult"),
                         in_channels=get_param(arch_params, "in_channels", 3))
