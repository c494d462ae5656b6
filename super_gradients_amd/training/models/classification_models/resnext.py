"""ResNeXt on the HIP kernels.

Reference: training/models/classification_models/resnext.py - GroupedConvBlock (:26-69), ResNeXt (:72-144), ResNeXt50 / ResNeXt101
(:158-167).  The ResNet bottleneck with a grouped 3x3 conv2 (csrc/gconv.h through GroupedConvLayer); stem, max-pool, block plumbing and
driver are resnet.py's.  Same state_dict keys as the reference: conv1.weight, bn1.*, layer{i}.{j}.{conv1,bn1,conv2,bn2,conv3,bn3},
layer{i}.{j}.downsample.{0,1}, fc.*; conv2.weight is [width, width / cardinality, 3, 3].
Not on the HIP path: replace_stride_with_dilation (dilated convolutions), networks of three layers.
"""
import torch

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import _conv_layer
from ....modules.classifier import num_classes_of
from ....modules.layers import BatchNorm, ConvLayer, LinearLayer, MaxPool, Numbered
from .resnet import ResBlock, ResNet, ResNetBase


class GroupedConvBlock(ResBlock):
    """Reference GroupedConvBlock: 1x1 -> grouped 3x3 (stride) -> 1x1, each with BatchNorm, ReLU after the first two and after the add."""

    expansion = 4
    final_relu = True

    def __init__(self, inplanes, planes, stride=1, groups=1, base_width=64, dilation=1):
        super().__init__()
        if dilation != 1:
            raise NotImplementedError("ResNeXt on the HIP path: dilation 1 (no dilated convolution kernels)")
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = ConvLayer(inplanes, width, 1, 1, 0, bias=False)
        self.bn1 = BatchNorm(width)
        self.conv2 = _conv_layer(width, width, 3, stride, 1, groups)
        self.bn2 = BatchNorm(width)
        self.conv3 = ConvLayer(width, planes * self.expansion, 1, 1, 0, bias=False)
        self.bn3 = BatchNorm(planes * self.expansion)
        self.downsample = Numbered()  # (the reference's None: an empty namespace adds no key)
        if stride != 1 or inplanes != planes * self.expansion:
            self.downsample.add_module("0", ConvLayer(inplanes, planes * self.expansion, 1, stride, 0, bias=False))
            self.downsample.add_module("1", BatchNorm(planes * self.expansion))
        self.stride = stride

    _folded = None  # {1: (filter with bn2's scale folded in, shift as bias)}: eval form of conv2, set by prep_model_for_conversion

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        """Eval form of the grouped layer as ONE launch: relu(gconv(x, w * s[k]) + t[k]) with bn2's running statistics folded in."""
        if not self.conv2.grouped:
            return
        w = self.conv2._w
        if w is None:
            raise RuntimeError("prep_model_for_conversion needs a materialised model (the fold reads the arena views)")
        with torch.no_grad():
            bn = self.bn2
            s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
            wf = K.ohwi_empty(*w.shape, w.device)
            wf.copy_(w.detach() * s.view(-1, 1, 1, 1))
            self._folded = {1: (wf, (bn.bias.detach() - bn.running_mean * s).contiguous())}

    def train(self, mode: bool = True):
        if mode:
            self._folded = None  # the weights are about to change
        return super().train(mode)

    @property
    def shortcut(self):  # ResBlock's name for it
        return self.downsample

    def _branch(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]


class ResNeXt(ResNet):
    _head_path = _finetune_key = "fc"

    def __init__(self, layers, cardinality, bottleneck_width, num_classes=10, replace_stride_with_dilation=None, in_channels: int = 3):
        ResNetBase.__init__(self)
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError("replace_stride_with_dilation should be None or a 3-element tuple, got {}".format(replace_stride_with_dilation))
        if any(replace_stride_with_dilation):
            raise NotImplementedError("ResNeXt on the HIP path: replace_stride_with_dilation is not available (no dilated convolution kernels)")
        if len(layers) != 4:
            raise NotImplementedError("ResNeXt on the HIP path: four layers")
        self.cardinality, self.base_width = cardinality, bottleneck_width
        self.inplanes = 64
        self.conv1 = ConvLayer(in_channels, self.inplanes, 7, 2, 3, bias=False)
        self.bn1 = BatchNorm(self.inplanes)
        self.maxpool = MaxPool(3, 2, 1)
        self.layer1 = self._make_group(64, layers[0], 1)
        self.layer2 = self._make_group(128, layers[1], 2)
        self.layer3 = self._make_group(256, layers[2], 2)
        self.layer4 = self._make_group(512, layers[3], 2)
        self.fc = LinearLayer(512 * GroupedConvBlock.expansion, num_classes)

    def _make_group(self, planes, blocks, stride):
        out = []
        for s in [stride] + [1] * (blocks - 1):
            out.append(GroupedConvBlock(self.inplanes, planes, s, self.cardinality, self.base_width))
            self.inplanes = planes * GroupedConvBlock.expansion
        return Numbered(out)


@register_model("resnext50")
class ResNeXt50(ResNeXt):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(layers=[3, 4, 6, 3], cardinality=32, bottleneck_width=4, num_classes=num_classes_of(arch_params, num_classes))


@register_model("resnext101")
class ResNeXt101(ResNeXt):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(layers=[3, 4, 23, 3], cardinality=32, bottleneck_width=8, num_classes=num_classes_of(arch_params, num_classes))
