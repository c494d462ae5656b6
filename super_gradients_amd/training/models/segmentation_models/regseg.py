"""RegSeg's backbone block on the HIP kernels.

Reference: training/models/segmentation_models/regseg.py - SqueezeAndExcitationBlock (:58-71), AdaptiveShortcutBlock (:74-92),
SplitDilatedGroupConvBlock (:95-122), DBlock (:125-171).  Same constructor arguments and state_dict keys (shortcut.shortcut.1.seq.{conv,bn}.*,
d_block_path.{0,5}.seq.{conv,bn}.*, d_block_path.1.weight or d_block_path.1.convs.{i}.weight, d_block_path.2.*,
d_block_path.4.se_block.{1,3}.{weight,bias}), so block checkpoints interchange both ways.

Kernel sequence of a DBlock (training):
    1x1 conv (BatchNorm statistics from its epilogue) -> bn_finalize -> affine + ReLU sweep
    dilated conv: ONE sgx_dgconv3x3_fwd launch over all splits (dilations [1]: sgx_gconv3x3_fwd, stride 1 / 2), statistics in its launch
        -> bn_finalize -> affine + ReLU sweep                                                               [a, stored]
    SE: image_colsum(a) -> 1x1 conv + bias + ReLU -> 1x1 conv + bias (both on [N,1,1,C]) -> channel_gate(a, pre, sigmoid)
    1x1 conv -> bn_finalize;  shortcut: identity, or [2x2 ceil-mode average pool ->] 1x1 conv -> bn_finalize -> affine sweep
    out = relu(bn(t) + shortcut)                                                                             one sweep
Against the reference's split -> n convolutions -> cat, the dilated convolution reads and writes the map once.


Around the blocks (RegSegBackbone :221-251, RegSegDecoder :174-202, RegSegHead :205-218, RegSeg :254-310, RegSeg48 :313-325), with the
reference's keys (stem.seq.*, backbone.stages.{i}.{str(block)}#{j}.*, decoder.projections.{i}.seq.*, decoder.conv_bn_relu.seq.*,
head.head.0.seq.*, head.head.1.{weight,bias}):
    decoder: proj1 + upsample(proj2) is ONE bilinear launch with proj1 as its addend; torch.cat((up(proj1), proj0)) has no concat pass -
        the second up-sampling and proj0's BatchNorm sweep write the two channel slices (offset 64) of one buffer.
    head: 3x3 conv -> BN -> ReLU, the class-count 1x1 convolution with bias, then sgx_bilinear_nchw_fwd: the x4 up-sampling and the
        NHWC -> NCHW layout change in one pass; the network returns the contiguous NCHW logits.
The stem's convolution has a bias in front of its BatchNorm, as the reference's: statistics are taken of conv + bias in the epilogue.

Not built (each raises NotImplementedError): RegSeg53 (group width 24, unregistered in the reference); stride 2 together with a dilation above
1 (RegSeg never combines them); head dropout > 0; half-precision inference; nearest / other interpolation modes.
Training: CrossEntropyLoss on the NCHW logits and the PixelAccuracy / IoU metrics run on csrc/segloss.h.
"""
from typing import Dict

import torch
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNReLU, ConvBNView, _ConvBN, _Seq
from ....modules.engine import SgxBlock, SgxNetwork
from ....modules.layers import (AvgPool2Ceil, BatchNorm, BilinearUpsample, ConvLayer, DilatedGroupedConvLayer, GroupedConvLayer, Numbered,
                                 widen_conv_input)
from ....modules.se_blocks import ConvSqueezeExcite, _SEConv
from ...utils.utils import get_param
from ..detection_models.yolo_nas.dfl_heads import _PredConv

DEFAULT_REGSEG48_BACKBONE_PARAMS = {
    "stages": [
        [[48, [1], 16, 2, 4]],
        [[128, [1], 16, 2, 4], *[[128, [1], 16, 1, 4]] * 2],
        [
            [256, [1], 16, 2, 4],
            [256, [1], 16, 1, 4],
            [256, [1, 2], 16, 1, 4],
            *[[256, [1, 4], 16, 1, 4]] * 4,
            *[[256, [1, 14], 16, 1, 4]] * 6,
            [320, [1, 14], 16, 1, 4],
        ],
    ]
}
DEFAULT_REGSEG48_DECODER_PARAMS = {"projection_out_channels": [8, 128, 128], "interpolation": "bilinear"}
DEFAULT_REGSEG_HEAD_PARAMS = {"dropout": 0.0, "interpolation": "bilinear", "align_corners": False, "upsample_factor": 4}
DEFAULT_REGSEG48_HEAD_PARAMS = {"mid_channels": 64, **DEFAULT_REGSEG_HEAD_PARAMS}


class SqueezeAndExcitationBlock(ConvSqueezeExcite):
    """x * sigmoid(conv2(relu(conv1(mean_hw(x))))); keys se_block.1.* / se_block.3.* as in the reference's nn.Sequential."""

    def __init__(self, in_channels, bottleneck_channels):
        super().__init__(in_channels, bottleneck_channels)
        self.se_block = Numbered(**{"1": _SEConv(in_channels, bottleneck_channels), "3": _SEConv(bottleneck_channels, in_channels)})

    def _convs(self):
        return self.se_block._modules["1"], self.se_block._modules["3"]


class AdaptiveShortcutBlock(SgxBlock):
    """Ceil-mode 2x2 average pool when stride is 2, then a 1x1 conv + BatchNorm when the widths differ or the map was pooled; otherwise the
    identity (`identity` is True and the owner adds x itself)."""

    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        if stride not in (1, 2):
            raise NotImplementedError(f"AdaptiveShortcutBlock on the HIP path: stride 1 or 2, got {stride}")
        self.identity = stride == 1 and in_channels == out_channels
        self.shortcut = Numbered()
        if stride != 1:
            self.shortcut.add_module("0", AvgPool2Ceil())
        if not self.identity:
            self.shortcut.add_module("1", ConvBNReLU(in_channels, out_channels, kernel_size=1, bias=False, use_activation=False))

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        if self.identity:
            return x
        pool = self.shortcut._modules.get("0")
        return self.shortcut._modules["1"].fwd(pool.fwd(x) if pool is not None else x, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        pool = self.shortcut._modules.get("0")
        if pool is None:
            return self.shortcut._modules["1"].bwd(dy, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        d = self.shortcut._modules["1"].bwd(dy, need_dx=need_dx)
        return pool.bwd(d, dx_out=dx_out, accumulate=accumulate) if need_dx else None


class SplitDilatedGroupConvBlock(DilatedGroupedConvLayer):
    """The reference's split -> one dilated grouped convolution per split -> cat, as one launch; keys convs.{i}.weight."""

    def __init__(self, in_channels, split_dilations, group_width_per_split, stride, bias):
        if stride != 1 or bias:
            raise NotImplementedError("SplitDilatedGroupConvBlock on the HIP path: stride 1, bias=False")
        if len(split_dilations) < 2:
            raise NotImplementedError("SplitDilatedGroupConvBlock holds two or more splits (one dilation is DBlock's plain convolution)")
        super().__init__(in_channels, split_dilations, group_width_per_split)


class _ConvBNPair(ConvBNView):
    """The dilated convolution and the BatchNorm + ReLU behind it (d_block_path.1 / .2); eval keeps the unfolded sequence."""

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        pass


class DBlock(SgxBlock):
    def __init__(self, in_channels, out_channels, dilations, group_width, stride, se_ratio=4):
        super().__init__()
        dilations = [int(d) for d in dilations]
        if group_width != 16:
            raise NotImplementedError(f"DBlock on the HIP path: group width 16 (RegSeg53's 24 is not built), got {group_width}")
        if stride != 1 and dilations != [1]:
            raise NotImplementedError("DBlock on the HIP path: stride 2 goes with dilations [1] only")
        self.in_channels, self.out_channels, self.dilations = in_channels, out_channels, dilations
        self.group_width, self.stride, self.se_ratio = group_width, stride, se_ratio
        self.shortcut = AdaptiveShortcutBlock(in_channels, out_channels, stride)
        if dilations == [1]:
            dilated = GroupedConvLayer(out_channels, out_channels // group_width, stride)
        elif len(dilations) == 1:
            dilated = DilatedGroupedConvLayer(out_channels, dilations, group_width)
        else:
            dilated = SplitDilatedGroupConvBlock(out_channels, dilations, group_width, stride, bias=False)
        self.d_block_path = Numbered(**{
            "0": ConvBNReLU(in_channels, out_channels, kernel_size=1, bias=False),
            "1": dilated,
            "2": BatchNorm(out_channels),
            "4": SqueezeAndExcitationBlock(out_channels, in_channels // se_ratio),
            "5": ConvBNReLU(out_channels, out_channels, 1, use_activation=False, bias=False),
        })
        self._mid = _ConvBNPair(dilated, self.d_block_path._modules["2"], "relu")

    def __str__(self):
        return f"{self.__class__.__name__}_in{self.in_channels}_out{self.out_channels}_d{self.dilations}_gw{self.group_width}_s{self.stride}_se{self.se_ratio}"

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        path = self.d_block_path._modules
        a = path["4"].fwd(self._mid.fwd(path["0"].fwd(x)))
        short = self.shortcut.fwd(x)
        conv3, bn3 = path["5"]._parts()
        if self.training:
            t, parts = conv3.conv(a, stats=True)
            sc, sh, mean, invstd = bn3.scale_shift(parts, t.shape[0] * t.shape[1] * t.shape[2], True)
        else:
            t = conv3.conv(a)
            sc, sh, mean, invstd = bn3.scale_shift(None, 0, False)
        y = K.affine_act(t, sc, sh, r1=short, a1=1.0, act="relu", out=out)
        self._ctx = (a, t, sc, sh, mean, invstd, y) if self.training else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (a, t, sc, sh, mean, invstd, y), self._ctx = self._ctx, None
        if addend is not None:
            raise NotImplementedError("DBlock.bwd: no addend (the shortcut uses the first data gradient's)")
        path = self.d_block_path._modules
        conv3, bn3 = path["5"]._parts()
        g = K.relu_bwd(dy, y)
        dt = bn3.backward(g, t, sc, sh, mean, invstd, None, dx_out=t)
        conv3.wgrad(a, dt)
        d = self._mid.bwd(path["4"].bwd(conv3.dgrad(dt, tuple(a.shape))))
        if self.shortcut.identity:  # + g in the first data gradient's epilogue
            return path["0"].bwd(d, dx_out=dx_out, accumulate=accumulate, addend=g, need_dx=need_dx)
        dx = path["0"].bwd(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        return self.shortcut.bwd(g, dx_out=dx, accumulate=True, need_dx=need_dx)


class RegSegStem(_ConvBN):
    """The reference's ConvBNReLU(3, 32, 3, stride=2, padding=1) with its default bias=True: keys seq.conv.{weight,bias}, seq.bn.*.  The
    BatchNorm statistics are those of conv + bias (the convolution's epilogue emits them after the bias); eval keeps the unfolded sequence."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.seq = _Seq()
        self.seq.add_module("conv", ConvLayer(in_channels, out_channels, 3, 2, 1, bias=True))
        self.seq.add_module("bn", BatchNorm(out_channels))
        self.act = "relu"

    def _parts(self):
        return self.seq.conv, self.seq.bn

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        pass

    def get_input_channels(self):
        return self.seq.conv.in_channels


class RegSegBackbone(nn.Module):
    def __init__(self, in_channels, backbone_config):
        super().__init__()
        self.stages = Numbered()
        self.backbone_output_channels = []
        prev = in_channels
        for s, stage in enumerate(backbone_config["stages"]):
            blocks = Numbered()
            for i, (out_channels, dilations, group_width, stride, se_ratio) in enumerate(stage):
                blk = DBlock(prev, out_channels, dilations, group_width, stride, se_ratio)
                prev = out_channels
                blocks.add_module(f"{str(blk)}#{i}", blk)  # (the reference's names: {i} distinguishes equal blocks)
            self.stages.add_module(str(s), blocks)
            self.backbone_output_channels.append(prev)

    def get_backbone_output_number_of_channels(self):
        return self.backbone_output_channels


class RegSegDecoder(SgxBlock):
    """Three stages in, mid // 2 + projection_out_channels[0] channels at the first stage's extent out (the paper's decoder)."""

    def __init__(self, backbone_output_channels, decoder_config):
        super().__init__()
        proj = decoder_config["projection_out_channels"]
        assert len(backbone_output_channels) == len(proj) == 3, "This decoder is specific for 3 stages"
        if decoder_config["interpolation"] != "bilinear":
            raise NotImplementedError(f"RegSegDecoder on the HIP path: bilinear interpolation, got {decoder_config['interpolation']}")
        self.projections = Numbered([ConvBNReLU(cin, cout, 1, bias=False) for cin, cout in zip(backbone_output_channels, proj)])
        self.upsample = BilinearUpsample(2, align_corners=True)
        mid = proj[1]
        self.conv_bn_relu = ConvBNReLU(in_channels=mid, out_channels=mid // 2, kernel_size=3, padding=1, bias=False)
        self._up_channels = mid // 2
        self.out_channels = mid // 2 + proj[0]

    def on_materialize(self):
        pass

    def fwd(self, x_stages, out=None):
        p0, p1, p2 = self.projections.blocks()
        s = self.upsample.fwd(p2.fwd(x_stages[2]), addend=p1.fwd(x_stages[1]))  # proj1 + up(proj2)
        c = self.conv_bn_relu.fwd(s)
        n, h, w, _ = x_stages[0].shape
        if out is None:
            out = torch.empty(n, h, w, self.out_channels, device=c.device, dtype=c.dtype)
        self.upsample.fwd(c, out=out[..., : self._up_channels])                     # cat((up(proj1), proj0)): two slices of one buffer
        p0.fwd(x_stages[0], out=out[..., self._up_channels:])
        return out

    def bwd_stages(self, dy):
        """-> the gradients of the three stage outputs"""
        p0, p1, p2 = self.projections.blocks()
        d0 = p0.bwd(dy[..., self._up_channels:])
        ds = self.conv_bn_relu.bwd(self.upsample.bwd(dy[..., : self._up_channels]))
        d2 = p2.bwd(self.upsample.bwd(ds))
        d1 = p1.bwd(ds)
        return d0, d1, d2


class RegSegHead(SgxBlock):
    def __init__(self, in_channels, num_classes, head_config):
        super().__init__()
        if head_config["dropout"] > 0:
            raise NotImplementedError("RegSegHead on the HIP path: dropout > 0 is not built")
        if head_config["interpolation"] != "bilinear":
            raise NotImplementedError(f"RegSegHead on the HIP path: bilinear interpolation, got {head_config['interpolation']}")
        self.num_classes = num_classes
        self.scale, self.align_corners = int(head_config["upsample_factor"]), bool(head_config["align_corners"])
        self.head = Numbered([ConvBNReLU(in_channels, head_config["mid_channels"], 3, bias=False, padding=1),
                              _PredConv(head_config["mid_channels"], num_classes, 1, bias=True)])  # (any class count: its backward pads to 4)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        cbr, cls = self.head.blocks()
        return K.bilinear_nchw_fwd(cls.fwd(cbr.fwd(x)), self.scale, self.align_corners)  # NHWC logits -> the contiguous NCHW map

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        cbr, cls = self.head.blocks()
        dl = K.bilinear_nchw_bwd(dy.contiguous(), self.scale, self.align_corners)
        return cbr.bwd(cls.bwd(dl), dx_out=dx_out, accumulate=accumulate)


class RegSeg(SgxNetwork):
    def __init__(self, stem, backbone, decoder, head):
        super().__init__()
        self.stem, self.backbone, self.decoder, self.head = stem, backbone, decoder, head

    def _stages(self):
        return [(f"backbone.stages.{name}.", st.blocks()) for name, st in self.backbone.stages._modules.items()]

    def _fwd(self, x):
        cin = self.get_input_channels()
        if x.dim() != 4 or x.shape[1] != cin:
            raise ValueError(f"expected an NCHW batch with {cin} channels, got {tuple(x.shape)}")
        a = self.stem.fwd(K.input_to_nhwc(x))
        outs = []
        for _, blocks in self._stages():
            for blk in blocks:
                a = blk.fwd(a)
            outs.append(a)
        return (self.head.fwd(self.decoder.fwd(outs)),)

    def _bwd(self, d_out):
        ready = self._bucket_ready
        d = self.head.bwd(d_out)
        ready("head.")
        skips = list(self.decoder.bwd_stages(d))
        ready("decoder.")
        stages = self._stages()
        d = skips[2]
        for s in range(2, -1, -1):
            prefix, blocks = stages[s]
            for i in range(len(blocks) - 1, 0, -1):
                d = blocks[i].bwd(d)
            if s:  # the stage's input is the previous stage's output: its decoder gradient is the tensor this gradient is added to
                d = blocks[0].bwd(d, dx_out=skips[s - 1], accumulate=True)
            else:
                d = blocks[0].bwd(d)
            ready(prefix)
        self.stem.bwd(d, need_dx=False)
        ready("stem.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["stem."] + [p for p, _ in self._stages()] + ["decoder.", "head."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def initialize_param_groups(self, lr, training_params) -> list:
        multiply_head_lr = get_param(training_params, "multiply_head_lr", 1)
        named = list(self.named_parameters())
        return [{"named_params": [(n, p) for n, p in named if "head." not in n], "lr": lr, "name": "no_multiply_params"},
                {"named_params": [(n, p) for n, p in named if "head." in n], "lr": lr * multiply_head_lr, "name": "multiply_lr_params"}]

    def update_param_groups(self, param_groups, lr, epoch, iter, training_params, total_batch) -> list:
        multiply_head_lr = get_param(training_params, "multiply_head_lr", 1)
        for group in param_groups:
            group["lr"] = lr * (multiply_head_lr if group["name"] == "multiply_lr_params" else 1)
        return param_groups

    def replace_head(self, new_num_classes, head_config=None):
        if self._materialized:
            raise RuntimeError("replace_head must be called before the model is materialized in HBM")
        self.head = RegSegHead(self.decoder.out_channels, new_num_classes, head_config or self._head_config)

    def get_finetune_lr_dict(self, lr: float) -> Dict[str, float]:
        return {"head": lr, "default": 0}

    def replace_input_channels(self, in_channels, compute_new_weights_fn=None):
        if self._materialized:
            raise RuntimeError("replace_input_channels must be called before the model is materialized in HBM (before the first forward)")
        self.stem.seq.conv = widen_conv_input(self.stem.seq.conv, in_channels, compute_new_weights_fn)

    def get_input_channels(self) -> int:
        return self.stem.get_input_channels()


@register_model("regseg48")
class RegSeg48(RegSeg):
    _head_config = DEFAULT_REGSEG48_HEAD_PARAMS

    def __init__(self, arch_params, num_classes=None):
        num_classes = num_classes or get_param(arch_params, "num_classes")
        backbone = RegSegBackbone(32, DEFAULT_REGSEG48_BACKBONE_PARAMS)
        decoder = RegSegDecoder(backbone.get_backbone_output_number_of_channels(), DEFAULT_REGSEG48_DECODER_PARAMS)
        super().__init__(RegSegStem(3, 32), backbone, decoder, RegSegHead(decoder.out_channels, num_classes, DEFAULT_REGSEG48_HEAD_PARAMS))


class RegSeg53(RegSeg):
    def __init__(self, arch_params, num_classes=None):
        raise NotImplementedError("RegSeg53 is not on the HIP path: its group width is 24 (the dilated kernels are built for 16), and the reference "
                                  "does not register it")
