"""RegNet / AnyNet classifiers on the HIP kernels.

Reference: training/models/classification_models/regnet.py - Head (:21-33), Stem (:36-55), XBlock (:58-106), Stage (:109-119), AnyNetX
(:122-190), regnet_params_to_blocks (:193-208), RegNetX / RegNetY (:211-243), verify_correctness_of_parameters (:246-256) and the seven
registered classes (:259-335).  Same constructor arguments, parameter arithmetic, initial weight distributions and state_dict keys
(net.stem.{conv,bn}.*, net.stage_{i}.blocks.block_{j}.{conv_block_1,conv_block_2,conv_block_3,shortcut}.{0,1}.*, ...se.{1,3}.{weight,bias},
net.head.fc.*), so checkpoints interchange both ways.

Kernel sequence of an XBlock (training; DESIGN.md 17 counts the passes):
    1x1 conv (BatchNorm statistics from its epilogue) -> bn_finalize -> affine + ReLU sweep
    grouped 3x3 conv, stride 1 / 2 (csrc/gconv.h, statistics in its launch) -> bn_finalize -> affine + ReLU sweep  [a, stored]
    SE: image_colsum(a) -> 1x1 conv + bias + ReLU -> 1x1 conv + bias (both on [N,1,1,C]) -> channel_gate(a, pre, sigmoid)
    1x1 conv -> bn_finalize;  shortcut: identity, or 1x1 conv (stride) -> bn_finalize -> affine sweep
    out = relu(bn3(t3) + shortcut)                                                                    one sweep
The SE hidden width is the block's INPUT width // se_ratio (the reference's rule), often no multiple of 4 (6, 38, 94 ...): it is padded to
the next multiple of 4 inside with zero filter rows / bias in the first convolution and zero columns in the second; parameters and gradients
keep the reference's shapes.  Eval after prep_model_for_conversion(): every conv + BatchNorm folds - the grouped layer is ONE
act(gconv + bias) launch, the last 1x1 takes the shortcut as its addend and the ReLU in its epilogue.

Not built (each raises NotImplementedError): droppath_prob > 0 (DropPath), replace_head(new_head=...), grouped layers whose channels per
group are outside the kernels' set.
"""
import numpy as np
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import Conv, ConvBNSeq
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import (ConvLayer, DepthwiseConvLayer, Dropout, GroupedConvLayer, LinearLayer, Numbered, init_normal_fan_out,
                                 widen_conv_input)
from ....modules.se_blocks import ConvSqueezeExcite, _SEConv
from ...utils.utils import get_param


class SqueezeExcite(ConvSqueezeExcite):
    """XBlock.se (regnet.py:71-81): x * sigmoid(conv2(relu(conv1(mean_hw(x))))); keys 1.weight / 1.bias / 3.weight / 3.bias as in the
    reference's nn.Sequential (0: pool, 2: ReLU, 4: Sigmoid, 5: Residual hold no state).  The arithmetic - hidden widths padded to a
    multiple of 4 inside - is modules/se_blocks.py's ConvSqueezeExcite."""

    def __init__(self, channels, hidden):
        super().__init__(channels, hidden)
        self.add_module("1", _SEConv(channels, hidden))
        self.add_module("3", _SEConv(hidden, channels))

    def _convs(self):
        return self._modules["1"], self._modules["3"]


class Stem(Conv):
    """Conv2d(in, out, 3, stride 2, pad 1, bias=False) + BatchNorm + ReLU; keys conv.weight, bn.*."""

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, out_channels, 3, 2, "relu", padding=1)

    def get_input_channels(self) -> int:
        return self.conv.in_channels


class XBlock(SgxBlock):
    def __init__(self, in_channels, out_channels, bottleneck_ratio, group_width, stride, se_ratio=None, droppath_prob=0.0):
        super().__init__()
        if droppath_prob:
            raise NotImplementedError("DropPath (droppath_prob > 0) is not on the HIP path")
        inter_channels = int(out_channels // bottleneck_ratio)
        groups = int(inter_channels // group_width)
        self.conv_block_1 = ConvBNSeq(in_channels, inter_channels, 1, activation_type="relu")
        self.conv_block_2 = ConvBNSeq(inter_channels, inter_channels, 3, stride=stride, padding=1, activation_type="relu", groups=groups)
        self.se = SqueezeExcite(inter_channels, in_channels // se_ratio) if se_ratio is not None else None
        self.conv_block_3 = ConvBNSeq(inter_channels, out_channels, 1)
        self.shortcut = ConvBNSeq(in_channels, out_channels, 1, stride=stride) if (stride != 1 or in_channels != out_channels) else None

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        a = self.conv_block_2.fwd(self.conv_block_1.fwd(x))
        if self.se is not None:
            a = self.se.fwd(a)
        short = self.shortcut.fwd(x) if self.shortcut is not None else x
        conv3, bn3 = self.conv_block_3._parts()
        folded = self.conv_block_3._folded
        if not self.training and folded is not None:
            return K.conv2d_fwd(a, folded[0], bias=folded[1], addend=short, out=out, act="relu")
        if self.training:
            self.conv_block_3._folded = None
            t, parts = conv3.conv(a, stats=True)
            sc, sh, mean, invstd = bn3.scale_shift(parts, t.shape[0] * t.shape[1] * t.shape[2], True)
        else:
            t = conv3.conv(a)
            sc, sh, mean, invstd = bn3.scale_shift(None, 0, False)
        y = K.affine_act(t, sc, sh, r1=short, a1=1.0, act="relu", out=out)
        self._ctx = (x, a, t, sc, sh, mean, invstd, y) if self.training else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, a, t, sc, sh, mean, invstd, y), self._ctx = self._ctx, None
        if addend is not None:
            raise NotImplementedError("XBlock.bwd: no addend (the shortcut uses the first data gradient's)")
        conv3, bn3 = self.conv_block_3._parts()
        g = K.relu_bwd(dy, y)
        dt = bn3.backward(g, t, sc, sh, mean, invstd, None, dx_out=t)
        conv3.wgrad(a, dt)
        d = conv3.dgrad(dt, tuple(a.shape))
        if self.se is not None:
            d = self.se.bwd(d)
        d = self.conv_block_2.bwd(d)
        if self.shortcut is None:  # identity: + g in the first data gradient's epilogue
            return self.conv_block_1.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=g, need_dx=need_dx)
        dx = self.conv_block_1.bwd(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        return self.shortcut.bwd(g, dx_out=dx, accumulate=True, need_dx=need_dx)


class Stage(nn.Module):
    def __init__(self, num_blocks, in_channels, out_channels, bottleneck_ratio, group_width, stride, se_ratio, droppath_prob):
        super().__init__()
        self.blocks = Numbered()
        self.blocks.add_module("block_0", XBlock(in_channels, out_channels, bottleneck_ratio, group_width, stride, se_ratio, droppath_prob))
        for i in range(1, num_blocks):
            self.blocks.add_module("block_{}".format(i), XBlock(out_channels, out_channels, bottleneck_ratio, group_width, 1, se_ratio, droppath_prob))


class Head(nn.Module):
    """Global average pool -> dropout (Philox mask, regenerated in the backward) -> Linear; key fc.*."""

    def __init__(self, num_channels, num_classes, dropout_prob):
        super().__init__()
        self.dropout = Dropout(dropout_prob)
        self.fc = LinearLayer(num_channels, num_classes)


class AnyNetX(SgxClassifier):
    _head_path, _finetune_key = "net.head.fc", "net.head"

    def __init__(self, ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width, stride, num_classes, se_ratio, backbone_mode,
                 dropout_prob=0.0, droppath_prob=0.0, input_channels=3):
        super().__init__()
        if droppath_prob:
            raise NotImplementedError("DropPath (droppath_prob > 0) is not on the HIP path")
        verify_correctness_of_parameters(ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width)
        self.net = Numbered()  # (children carry the reference's names: net.stem, net.stage_0 ..., net.head)
        self.backbone_mode = backbone_mode
        prev_block_width = 32
        self.net.add_module("stem", Stem(in_channels=input_channels, out_channels=prev_block_width))
        for i, (num_blocks, block_width, bottleneck_ratio, group_width) in enumerate(zip(ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width)):
            self.net.add_module("stage_{}".format(i), Stage(int(num_blocks), prev_block_width, int(block_width), bottleneck_ratio, int(group_width), stride, se_ratio,
                                                            droppath_prob))
            prev_block_width = int(block_width)
        if not self.backbone_mode:  # backbone mode: no head (average pool + fc)
            self.net.add_module("head", Head(int(ls_block_width[-1]), num_classes, dropout_prob))
        self.ls_block_width = [int(w) for w in ls_block_width]
        self.dropout_prob = dropout_prob
        self.initialize_weight()

    def initialize_weight(self):
        """Reference :157-167: conv weights N(0, sqrt(2 / (k * k * out_channels))), BatchNorm 1 / 0, linear N(0, 0.01) with zero bias.
        (The SE convolutions are nn.Conv2d too: the same normal draw; their biases keep nn.Conv2d's default.)"""
        init_normal_fan_out(self, (ConvLayer, DepthwiseConvLayer, GroupedConvLayer, _SEConv))

    def _blocks(self):
        return [(f"net.{sname}.", blk) for sname, st in self.net._modules.items() if isinstance(st, Stage) for blk in st.blocks.children_list()]

    def _fwd(self, x):
        a = self.net.stem.fwd(self._input_nhwc(x))
        for _, blk in self._blocks():
            a = blk.fwd(a)
        if self.backbone_mode:
            return (K.nhwc_to_nchw(a),)
        head = self.net.head
        return (self._pool_head_fwd(a, head.fc, head.dropout.p),)

    def _bwd(self, d_out):
        ready = self._bucket_ready
        if self.backbone_mode:
            d = K.nchw_to_nhwc(d_out)
        else:
            d = self._pool_head_bwd(d_out, self.net.head.fc)
            ready("net.head.")
        blocks = self._blocks()
        for i in range(len(blocks) - 1, -1, -1):
            prefix, blk = blocks[i]
            d = blk.bwd(d)
            if i == 0 or blocks[i - 1][0] != prefix:
                ready(prefix)
        self.net.stem.bwd(d, need_dx=False)
        ready("net.stem.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return [f"net.{name}." for name in self.net._modules]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def _new_head(self, new_num_classes):
        head = Head(self.ls_block_width[-1], new_num_classes, self.dropout_prob)
        head.fc.weight.data.normal_(mean=0.0, std=0.01)
        head.fc.bias.data.zero_()
        self.net.head = head

    def replace_input_channels(self, in_channels: int, compute_new_weights_fn=None):
        """Reference regnet.py:49-52, 181-183 with modules/weight_replacement_utils.py: the stem keeps the weights of the channels it already
        has; extra channels are drawn from a normal distribution with the old weights' mean / std.  Before materialisation only."""
        if self._materialized:
            raise RuntimeError("replace_input_channels must be called before the model is materialized in HBM (before the first forward)")
        self.net.stem.conv = widen_conv_input(self.net.stem.conv, in_channels, compute_new_weights_fn)

    def get_input_channels(self) -> int:
        return self.net.stem.get_input_channels()


def regnet_params_to_blocks(initial_width, slope, quantized_param, network_depth, bottleneck_ratio, group_width):
    """Block widths and counts from the RegNet parameters (the paper's equations 2 and 3, widths rounded to multiples of 8, then made
    compatible with the group width) - the reference's arithmetic, operation by operation."""
    parameterized_width = initial_width + slope * np.arange(network_depth)
    parameterized_block = np.log(parameterized_width / initial_width) / np.log(quantized_param)
    parameterized_block = np.round(parameterized_block)
    quantized_width = initial_width * np.power(quantized_param, parameterized_block)
    quantized_width = 8 * np.round(quantized_width / 8)
    ls_block_width, ls_num_blocks = np.unique(quantized_width.astype(np.int32), return_counts=True)
    ls_group_width = np.array([min(group_width, block_width // bottleneck_ratio) for block_width in ls_block_width])
    ls_block_width = (np.round(ls_block_width // bottleneck_ratio / group_width) * group_width).astype(np.int32).tolist()
    ls_bottleneck_ratio = [bottleneck_ratio for _ in range(len(ls_block_width))]
    return ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width.tolist()


def verify_correctness_of_parameters(ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width):
    """The parameters must fit the search space of the RegNet paper."""
    err_message = "Parameters don't fit"
    assert len(set(ls_bottleneck_ratio)) == 1, f"{err_message} AnyNetXb"
    assert len(set(ls_group_width)) == 1, f"{err_message} AnyNetXc"
    assert all(i <= j for i, j in zip(ls_block_width, ls_block_width[1:])) is True, f"{err_message} AnyNetXd"
    if len(ls_num_blocks) > 2:
        assert all(i <= j for i, j in zip(ls_num_blocks[:-2], ls_num_blocks[1:-1])) is True, f"{err_message} AnyNetXe"
    for block_width, bottleneck_ratio, group_width in zip(ls_block_width, ls_bottleneck_ratio, ls_group_width):
        assert int(block_width // bottleneck_ratio) % group_width == 0


class RegNetX(AnyNetX):
    def __init__(self, initial_width, slope, quantized_param, network_depth, bottleneck_ratio, group_width, stride, arch_params, se_ratio=None,
                 input_channels=3, num_classes=None):
        ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width = regnet_params_to_blocks(initial_width, slope, quantized_param, network_depth,
                                                                                                    bottleneck_ratio, group_width)
        super().__init__(ls_num_blocks, ls_block_width, ls_bottleneck_ratio, ls_group_width, stride, num_classes_of(arch_params, num_classes), se_ratio,
                         get_param(arch_params, "backbone_mode", False), get_param(arch_params, "dropout_prob", 0.0), get_param(arch_params, "droppath_prob", 0.0),
                         input_channels)


class RegNetY(RegNetX):
    """RegNetY = RegNetX + SE"""

    def __init__(self, initial_width, slope, quantized_param, network_depth, bottleneck_ratio, group_width, stride, arch_params, se_ratio, input_channels=3,
                 num_classes=None):
        super().__init__(initial_width, slope, quantized_param, network_depth, bottleneck_ratio, group_width, stride, arch_params, se_ratio, input_channels,
                         num_classes)


@register_model("custom_regnet")
class CustomRegNet(RegNetX):
    def __init__(self, arch_params, num_classes=None):
        """All parameters must be provided in arch_params other than SE"""
        g = lambda k: get_param(arch_params, k)  # noqa: E731
        super().__init__(initial_width=g("initial_width"), slope=g("slope"), quantized_param=g("quantized_param"), network_depth=g("network_depth"),
                         bottleneck_ratio=g("bottleneck_ratio"), group_width=g("group_width"), stride=g("stride"), arch_params=arch_params,
                         se_ratio=get_param(arch_params, "se_ratio", None), input_channels=get_param(arch_params, "input_channels", 3), num_classes=num_classes)


@register_model("custom_anynet")
class CustomAnyNet(AnyNetX):
    def __init__(self, arch_params, num_classes=None):
        """All parameters must be provided in arch_params other than SE"""
        g = lambda k: get_param(arch_params, k)  # noqa: E731
        super().__init__(ls_num_blocks=g("ls_num_blocks"), ls_block_width=g("ls_block_width"), ls_bottleneck_ratio=g("ls_bottleneck_ratio"),
                         ls_group_width=g("ls_group_width"), stride=g("stride"), num_classes=num_classes_of(arch_params, num_classes),
                         se_ratio=get_param(arch_params, "se_ratio", None), backbone_mode=get_param(arch_params, "backbone_mode", False),
                         dropout_prob=get_param(arch_params, "dropout_prob", 0), droppath_prob=get_param(arch_params, "droppath_prob", 0),
                         input_channels=get_param(arch_params, "input_channels", 3))


@register_model("nas_regnet")
class NASRegNet(RegNetX):
    def __init__(self, arch_params, num_classes=None):
        """All parameters are provided as a single structure list: arch_params.structure"""
        structure = get_param(arch_params, "structure")
        super().__init__(initial_width=structure[0], slope=structure[1], quantized_param=structure[2], network_depth=structure[3], bottleneck_ratio=structure[4],
                         group_width=structure[5], stride=structure[6], se_ratio=structure[7] if structure[7] > 0 else None, arch_params=arch_params,
                         num_classes=num_classes)


def _regnety(name, *params):
    def init(self, arch_params, num_classes=None):
        RegNetY.__init__(self, *params, 2, arch_params, 4, num_classes=num_classes)

    return register_model(name)(type("RegNetY" + name[7:], (RegNetY,), {"__init__": init}))


RegNetY200 = _regnety("regnetY200", 24, 36, 2.5, 13, 1, 8)
RegNetY400 = _regnety("regnetY400", 48, 28, 2.1, 16, 1, 8)
RegNetY600 = _regnety("regnetY600", 48, 33, 2.3, 15, 1, 16)
RegNetY800 = _regnety("regnetY800", 56, 39, 2.4, 14, 1, 16)
