"""MobileNetV2 classifiers on the HIP kernels.

Reference: training/models/classification_models/mobilenetv2.py - MobileNetBase (:23-36), InvertedResidual (:53-99), MobileNetV2 (:102-202),
MobileNetV2Base / MobileNetV2_135 / CustomMobileNetV2 (:205-254).  Same constructor arguments, structure table, `make_divisible` rule (and its
quirk: the t == 1 stages are not scaled by width_mult), last-channel rule, initial weight distributions and state_dict keys
(features.0.{0,1}.*, features.{i}.conv.{j}.*, features.{last}.{0,1}.*, classifier.1.*), so checkpoints interchange both ways.

Kernel sequence (training), per inverted residual: [1x1 expansion conv (statistics in its epilogue) -> bn_finalize -> affine + ReLU6 sweep]
-> depthwise 3x3 (sgx_dwconv3x3_fwd, statistics in its launch) -> bn_finalize -> affine + ReLU6 sweep -> 1x1 projection conv -> bn_finalize ->
affine sweep that also adds the block's input where the reference computes `x + conv(x)` (r1 of sgx_affine_act_fwd: the residual is not a
pass of its own).  Backward: BatchNorm backward -> weight gradient (side stream) -> data gradient, layer by layer; the residual's gradient
joins in the block's first data gradient (its addend).  Eval after prep_model_for_conversion(): every conv + BatchNorm folds into filter and
bias; the depthwise layers run as one launch act(dwconv + bias), the 1x1 layers as conv + bias followed by the ReLU6 sweep (the conv epilogues
do not carry ReLU6), the projection as conv + bias + residual in one launch.  Then global average pool -> linear, as in resnet.py.

Not built (each raises NotImplementedError): backbone_mode=True; grouped_conv_size != 1 (grouped, not depthwise, convolutions); widths
that are not multiples of 4 (16-byte channel groups); dropout > 0 in training mode (eval is the identity and works);
replace_head(new_head=...).
"""
import math

from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNSeq, ConvBNView
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, DepthwiseConvLayer, LinearLayer, Numbered, init_normal_fan_out, need_mult4
from ...utils.utils import get_param

DEFAULT_STRUCTURE = [
    # t (expansion), c (width), n (blocks), s (stride of the first block)
    [1, 16, 1, 1],
    [6, 24, 2, 2],
    [6, 32, 3, 2],
    [6, 64, 4, 2],
    [6, 96, 3, 1],
    [6, 160, 3, 2],
    [6, 320, 1, 1],
]


def make_divisible(x, divisible_by=8):
    return int(math.ceil(x * 1.0 / divisible_by) * divisible_by)


class InvertedResidual(SgxBlock):
    """Reference InvertedResidual: [1x1 expand, BN, ReLU6,] depthwise 3x3, BN, ReLU6, 1x1 project, BN - keys conv.{0..7} ({0..4} for t == 1)."""

    def __init__(self, inp, oup, stride, expand_ratio, grouped_conv_size=1):
        super().__init__()
        assert stride in (1, 2)
        if grouped_conv_size != 1:
            raise NotImplementedError("MobileNetV2 on the HIP path: grouped_conv_size=1 (depthwise); grouped convolutions are not built")
        hidden = int(inp * expand_ratio)
        need_mult4("MobileNetV2", "block input width", inp)
        need_mult4("MobileNetV2", "hidden width", hidden)
        need_mult4("MobileNetV2", "block output width", oup)
        self.stride = stride
        self.use_res_connect = stride == 1 and inp == oup
        if expand_ratio == 1:
            layers = {"0": DepthwiseConvLayer(hidden, stride), "1": BatchNorm(hidden), "3": ConvLayer(hidden, oup, 1, 1, 0), "4": BatchNorm(oup)}
            pw, dw, pwl = None, ("0", "1"), ("3", "4")
        else:
            layers = {"0": ConvLayer(inp, hidden, 1, 1, 0), "1": BatchNorm(hidden), "3": DepthwiseConvLayer(hidden, stride), "4": BatchNorm(hidden),
                      "6": ConvLayer(hidden, oup, 1, 1, 0), "7": BatchNorm(oup)}
            pw, dw, pwl = ("0", "1"), ("3", "4"), ("6", "7")
        self.conv = Numbered(**layers)
        # the conv -> BatchNorm -> activation sequences over those layers (they own no parameter: nothing is added to the state)
        self.pw = ConvBNView(layers[pw[0]], layers[pw[1]], "relu6") if pw else None
        self.dw = ConvBNView(layers[dw[0]], layers[dw[1]], "relu6")
        self.pwl = ConvBNView(layers[pwl[0]], layers[pwl[1]], None)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        a = self.pw.fwd(x) if self.pw is not None else x
        a = self.dw.fwd(a)
        return self.pwl.fwd(a, out=out, residual=x if self.use_res_connect else None)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        if addend is not None:
            raise NotImplementedError("InvertedResidual.bwd: no addend (the residual uses the first data gradient's)")
        res = dy if self.use_res_connect else None  # d(x + conv(x)) = dy + d conv: dy joins the block's first data gradient
        d = self.pwl.bwd(dy)
        first = self.pw if self.pw is not None else self.dw
        if first is not self.dw:
            d = self.dw.bwd(d)
        return first.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=res, need_dx=need_dx)


class MobileNetV2(SgxClassifier):
    _head_path, _finetune_key = "classifier.1", "classifier"

    def __init__(self, num_classes, dropout: float, width_mult=1.0, structure=None, backbone_mode: bool = False, grouped_conv_size=1, in_channels=3):
        super().__init__()
        if backbone_mode:
            raise NotImplementedError("MobileNetV2 on the HIP path: backbone_mode=False (MobileNet as a detection backbone is not built)")
        if grouped_conv_size != 1:
            raise NotImplementedError("MobileNetV2 on the HIP path: grouped_conv_size=1 (depthwise); grouped convolutions are not built")
        self.in_channels = in_channels
        self.interverted_residual_setting = structure or [list(r) for r in DEFAULT_STRUCTURE]  # (the reference's spelling)
        self.last_channel = make_divisible(1280 * width_mult) if width_mult > 1.0 else 1280
        self.backbone_mode, self.dropout = backbone_mode, float(dropout)
        curr = 32
        feats = [ConvBNSeq(in_channels, curr, 3, stride=2, padding=1, activation_type="relu6")]
        for t, c, n, s in self.interverted_residual_setting:
            oup = make_divisible(c * width_mult) if t > 1 else c
            for i in range(n):
                feats.append(InvertedResidual(curr, oup, s if i == 0 else 1, expand_ratio=t, grouped_conv_size=grouped_conv_size))
                curr = oup
        need_mult4("MobileNetV2", "the last block's width", curr)
        feats.append(ConvBNSeq(curr, self.last_channel, 1, stride=1, padding=0, activation_type="relu6"))
        self.features = Numbered(feats)
        self.classifier = Numbered(**{"1": LinearLayer(self.last_channel, num_classes)})  # ("0" is the reference's nn.Dropout: no state)
        init_normal_fan_out(self, (ConvLayer, DepthwiseConvLayer))  # (reference :180-193)

    def _fwd(self, x):
        a = self._input_nhwc(x)
        if self.training and self.dropout > 0:
            raise NotImplementedError("MobileNetV2 on the HIP path: dropout > 0 is not built for training (eval mode is the identity and works)")
        for f in self.features.blocks():
            a = f.fwd(a)
        return (self._pool_head_fwd(a, self.classifier._modules["1"]),)  # (the pool: the reference's x.mean(3).mean(2))

    def _bwd(self, d_logits):
        d = self._pool_head_bwd(d_logits, self.classifier._modules["1"])
        ready = self._bucket_ready
        ready("classifier.")
        feats = self.features.blocks()
        for i in range(len(feats) - 1, 0, -1):
            d = feats[i].bwd(d)
            ready(f"features.{i}.")
        feats[0].bwd(d, need_dx=False)
        ready("features.0.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return [f"features.{i}." for i in range(len(self.features.blocks()))] + ["classifier."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.features._modules["0"]._modules["0"].in_channels


@register_model("mobilenet_v2")
class MobileNetV2Base(MobileNetV2):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(num_classes=num_classes_of(arch_params, num_classes), width_mult=1.0, structure=None,
                         dropout=get_param(arch_params, "dropout", 0.0), in_channels=get_param(arch_params, "in_channels", 3))


@register_model("mobile_net_v2_135")
class MobileNetV2_135(MobileNetV2):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(num_classes=num_classes_of(arch_params, num_classes), width_mult=1.35, structure=None,
                         dropout=get_param(arch_params, "dropout", 0.0), in_channels=get_param(arch_params, "in_channels", 3))


@register_model("custom_mobilenet_v2")
class CustomMobileNetV2(MobileNetV2):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(num_classes=num_classes_of(arch_params, num_classes), width_mult=get_param(arch_params, "width_mult"),
                         structure=get_param(arch_params, "structure"), dropout=get_param(arch_params, "dropout", 0.0),
                         in_channels=get_param(arch_params, "in_channels", 3))
