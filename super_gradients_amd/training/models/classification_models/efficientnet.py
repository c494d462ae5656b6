"""EfficientNet classifiers on the HIP kernels.

Reference: training/models/classification_models/efficientnet.py - round_filters (:42-61), round_repeats (:64-75), drop_connect (:78-100),
the static "same" padding convolutions (:129-202), BlockDecoder (:222-300), MBConvBlock (:303-393), EfficientNet (:396-577),
get_efficientnet_params (:580-616) and the eleven registered classes (:619-842).  Same arch params and defaults (batch_norm_momentum 0.99 ->
BatchNorm momentum 0.01, eps 1e-3, drop_connect_rate 0.2, depth_divisor 8), the same block strings, the same rounding rules, nn.Conv2d /
nn.Linear default initial weight distributions and the same state_dict keys (_conv_stem.weight, _bn0.*, _blocks.{i}._expand_conv /
_bn0 / _depthwise_conv / _bn1 / _se_reduce / _se_expand / _project_conv / _bn2, _conv_head.weight, _bn1.*, _fc.*), so checkpoints interchange
both ways.

Kernel sequence of an MBConv block (training; DESIGN.md 18 counts the passes):
    [expand != 1: 1x1 conv (BatchNorm statistics from its epilogue) -> bn_finalize -> affine + SiLU sweep]
    depthwise 3x3 / 5x5, stride 1 / 2 (statistics in its launch) -> bn_finalize
    SE (after the activation): bn_act_gate_mean (reads the convolution output, stores no map) -> 1x1 conv + bias, SiLU, 1x1 conv + bias on
        [N,1,1,C] -> bn_act_gate_fwd: y = sigmoid(pre) * silu(bn1(t)) in one sweep.  silu(bn1(t)) is never stored.
    1x1 projection -> bn_finalize -> affine sweep (+ the residual; with drop-connect: bn_gate_add, the per-image multiplier in the same sweep)
Backward of the depthwise layer: bn_act_gate_bwd_gate (d pre), the two small convolutions' backward, bn_act_gate_bwd_data (dz and the
BatchNorm backward's reduce rows in one sweep), bn_bwd_finalize + bn_bwd_apply, the depthwise weight and data gradients.
Eval after prep_model_for_conversion(): every conv + BatchNorm folds; the depthwise layer is dwconv + bias in one launch followed by the
two gate sweeps without scale / shift.

Static "same" padding.  The reference pads from the CONFIGURED image_size, larger half first (ZeroPad2d((1, 0, 1, 0)) for 3x3 stride 2 on
an even size, (2, 1, 2, 1) for 5x5).  The kernels pad k // 2 on every side and produce ceil(H / s) rows.  Both read the same input window
for every output element whenever the reference's leading pad is k // 2 and the two output sizes agree: the trailing pad is then either
the same or never touched.  That holds for every layer of every variant except one situation - a strided layer configured for an even
size that receives an odd one (the reference then produces (H - 1) / 2 rows) - for which the forward raises NotImplementedError naming
the layer.  Each layer keeps the reference's pad tuple as `static_padding` (left, right, top, bottom).

Drop-connect (stochastic depth per image on the residual branch, identity-skip blocks in training only): block idx of n runs at rate
drop_connect_rate * idx / n.  The [N] multipliers (0 or 1 / keep) are sgx_dropout_fwd on a row of ones, its seed drawn from torch's default
generator (torch.manual_seed repeats a step), expanded to [N,C] - a copy of N * C floats, not a pass over the map - and applied by
bn_gate_add together with the BatchNorm affine and the residual.  The reference divides by keep where this multiplies by fl(1 / keep): at
most one ulp apart.  The mask differs from the reference's torch.rand draw; `MBConvBlock._test_keep_mask` ([N] of 0 / 1) injects one.

Reference quirk kept: the identity skip needs `block_args.stride == 1`, and BlockDecoder.decode yields stride=[1] (a list) - so a block
built straight from a decoded string never skips; EfficientNet's repeated blocks get stride=1 (an int) and do.

Not built (each raises NotImplementedError): image_size=None (dynamic same padding), the even-configured / odd-input mismatch above, widths
that are not multiples of 4, kernel sizes other than 3 / 5, replace_head(new_head=...); supports_half_inference() is False.
"""
import collections
import math
import re
from collections import OrderedDict
from typing import List

import torch
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNView
from ....modules.classifier import SgxClassifier
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, DepthwiseConvLayer, Dropout, LinearLayer, need_mult4, widen_conv_input
from ....modules.se_blocks import MBConvSE, _SEConv
from ...utils.utils import HpmStruct, get_param

BlockArgs = collections.namedtuple("BlockArgs", ["num_repeat", "kernel_size", "stride", "expand_ratio", "input_filters", "output_filters", "se_ratio", "id_skip"])
BlockArgs.__new__.__defaults__ = (None,) * len(BlockArgs._fields)


def round_filters(filters, width_coefficient, depth_divisor, min_depth):
    """Filter count under the width multiplier, rounded to depth_divisor, never more than 10 % below the scaled value."""
    if not width_coefficient:
        return filters
    filters *= width_coefficient
    min_depth = min_depth or depth_divisor
    new_filters = max(min_depth, int(filters + depth_divisor / 2) // depth_divisor * depth_divisor)
    if new_filters < 0.9 * filters:
        new_filters += depth_divisor
    return int(new_filters)


def round_repeats(repeats, depth_coefficient):
    if not depth_coefficient:
        return repeats
    return int(math.ceil(depth_coefficient * repeats))


def calculate_output_image_size(input_image_size, stride):
    if input_image_size is None:
        return None
    if isinstance(input_image_size, int):
        input_image_size = (input_image_size, input_image_size)
    h, w = input_image_size
    stride = stride if isinstance(stride, int) else stride[0]
    return [int(math.ceil(h / stride)), int(math.ceil(w / stride))]


class BlockDecoder(object):
    """Block strings such as 'r1_k3_s11_e1_i32_o16_se0.25_noskip' <-> BlockArgs."""

    @staticmethod
    def _decode_block_string(block_string: str) -> BlockArgs:
        assert isinstance(block_string, str)
        options = {}
        for op in block_string.split("_"):
            splits = re.split(r"(\d.*)", op)
            if len(splits) >= 2:
                options[splits[0]] = splits[1]
        assert ("s" in options and len(options["s"]) == 1) or (len(options["s"]) == 2 and options["s"][0] == options["s"][1])
        return BlockArgs(num_repeat=int(options["r"]), kernel_size=int(options["k"]), stride=[int(options["s"][0])], expand_ratio=int(options["e"]),
                         input_filters=int(options["i"]), output_filters=int(options["o"]), se_ratio=float(options["se"]) if "se" in options else None,
                         id_skip=("noskip" not in block_string))

    @staticmethod
    def _encode_block_string(block) -> str:
        args = ["r%d" % block.num_repeat, "k%d" % block.kernel_size, "s%d%d" % (block.strides[0], block.strides[1]), "e%s" % block.expand_ratio,
                "i%d" % block.input_filters, "o%d" % block.output_filters]
        if 0 < block.se_ratio <= 1:
            args.append("se%s" % block.se_ratio)
        if block.id_skip is False:
            args.append("noskip")
        return "_".join(args)

    @staticmethod
    def decode(string_list: List[str]) -> List[BlockArgs]:
        assert isinstance(string_list, list)
        return [BlockDecoder._decode_block_string(s) for s in string_list]

    @staticmethod
    def encode(blocks_args: List):
        return [BlockDecoder._encode_block_string(b) for b in blocks_args]


def _int_stride(stride):
    return stride if isinstance(stride, int) else stride[0]


class _SamePad:
    """The reference's static 'same' padding of one convolution (Conv2dStaticSamePadding.__init__), kept to check that the kernels'
    symmetric k // 2 padding computes the same thing on the input that actually arrives."""

    def __init__(self, name, kernel_size, stride, image_size):
        if image_size is None:
            raise NotImplementedError(f"EfficientNet on the HIP path: {name} needs a configured image_size (dynamic same padding, image_size=None, is not built)")
        ih, iw = (image_size, image_size) if isinstance(image_size, int) else image_size
        self.name, self.k, self.s = name, kernel_size, stride
        self.pad_h = max((math.ceil(ih / stride) - 1) * stride + kernel_size - ih, 0)
        self.pad_w = max((math.ceil(iw / stride) - 1) * stride + kernel_size - iw, 0)
        self.static_padding = (self.pad_w - self.pad_w // 2, self.pad_w // 2, self.pad_h - self.pad_h // 2, self.pad_h // 2)

    def check(self, h, w):
        half = self.k // 2
        for size, total, axis in ((h, self.pad_h, "height"), (w, self.pad_w, "width")):
            ref_out = (size + total - self.k) // self.s + 1
            own_out = (size + 2 * half - self.k) // self.s + 1
            if total - total // 2 != half or ref_out != own_out:
                raise NotImplementedError(f"EfficientNet on the HIP path: {self.name} ({self.k}x{self.k}, stride {self.s}) was configured for an even image "
                                          f"{axis} (static padding {self.static_padding}) and receives {size}: the reference then pads asymmetrically and "
                                          f"produces {ref_out} rows where the kernels' symmetric padding gives {own_out}")


class MBConvBlock(SgxBlock):
    """Mobile inverted residual bottleneck: [1x1 expand, BN, SiLU,] depthwise, BN, SiLU, [SE,] 1x1 project, BN [+ input]."""

    _test_keep_mask = None  # tests only: the [N] keep mask (0 / 1) the next drop-connect forward uses instead of its own Philox draw

    def __init__(self, block_args: BlockArgs, batch_norm_momentum: float, batch_norm_epsilon: float, image_size=None, name: str = "MBConvBlock"):
        super().__init__()
        self._block_args = block_args
        self._bn_mom = 1 - batch_norm_momentum  # pytorch's difference from tensorflow
        self._bn_eps = batch_norm_epsilon
        self.has_se = (block_args.se_ratio is not None) and (0 < block_args.se_ratio <= 1)
        self.id_skip = block_args.id_skip
        inp = block_args.input_filters
        oup = block_args.input_filters * block_args.expand_ratio
        final_oup = block_args.output_filters
        k, s = block_args.kernel_size, _int_stride(block_args.stride)
        if k not in (3, 5):
            raise NotImplementedError(f"EfficientNet on the HIP path: depthwise kernel size 3 or 5, got {k}")
        need_mult4("EfficientNet", "block input width", inp)
        need_mult4("EfficientNet", "expanded width", oup)
        need_mult4("EfficientNet", "block output width", final_oup)
        self._pad = _SamePad(f"{name}._depthwise_conv", k, s, image_size)
        bn = lambda c: BatchNorm(c, eps=self._bn_eps, momentum=self._bn_mom)  # noqa: E731
        self._pw = None
        if block_args.expand_ratio != 1:
            self._expand_conv = ConvLayer(inp, oup, 1, 1, 0, bias=False)
            self._bn0 = bn(oup)
            self._pw = ConvBNView(self._expand_conv, self._bn0, "silu")
        self._depthwise_conv = DepthwiseConvLayer(oup, s, k)
        self._bn1 = bn(oup)
        se = None
        if self.has_se:
            squeezed = max(1, int(block_args.input_filters * block_args.se_ratio))
            self._se_reduce = _SEConv(oup, squeezed)
            self._se_expand = _SEConv(squeezed, oup)
            se = MBConvSE(self._se_reduce, self._se_expand)
        self._se = se
        self._dw = ConvBNView(self._depthwise_conv, self._bn1, "silu", gate=se)
        self._project_conv = ConvLayer(oup, final_oup, 1, 1, 0, bias=False)
        self._bn2 = bn(final_oup)
        self._pwl = ConvBNView(self._project_conv, self._bn2, None)
        # (the reference's comparison, list or int as the block was given it: see the module docstring)
        self._skip = bool(self.id_skip and block_args.stride == 1 and inp == final_oup)

    @property
    def static_padding(self):
        return self._pad.static_padding

    def on_materialize(self):
        pass

    def _multipliers(self, n, c, p, dev):
        """[N, C] rows of 0 or 1 / keep: one Philox draw per image, expanded"""
        if self._test_keep_mask is not None:
            m = torch.as_tensor(self._test_keep_mask, dtype=torch.float32, device=dev).view(n) * (1.0 / (1.0 - p))
        else:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # torch's default generator: torch.manual_seed repeats a step
            np4 = (n + 3) // 4 * 4
            m = K.dropout(torch.ones(1, np4, device=dev), p, seed).view(np4)[:n]
        return m.view(n, 1).expand(n, c).contiguous()

    def fwd(self, x, out=None, drop_connect_rate=None):
        self._pad.check(x.shape[1], x.shape[2])
        a = self._pw.fwd(x) if self._pw is not None else x
        a = self._dw.fwd(a)
        self._dc = None
        if not (self._skip and self.training and drop_connect_rate):
            return self._pwl.fwd(a, out=out, residual=x if self._skip else None)
        assert 0 <= drop_connect_rate <= 1, "p must be in range of [0,1]"
        conv, bn = self._pwl._parts()
        self._pwl._folded = None
        t, parts = conv.conv(a, stats=True)
        n, h, w, c = t.shape
        sc, sh, mean, invstd = bn.scale_shift(parts, n * h * w, True)
        mult = self._multipliers(n, c, float(drop_connect_rate), t.device)
        self._dc = (a, t, sc, sh, mean, invstd, mult)
        return K.bn_gate_add(t, sc, sh, mult, "none", x, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        if addend is not None:
            raise NotImplementedError("MBConvBlock.bwd: no addend (the residual uses the first data gradient's)")
        res = dy if self._skip else None  # d(x + branch(x)) = dy + d branch: dy joins the block's first data gradient
        if self._dc is not None:  # m[n] * dy and the BatchNorm backward's reduce rows in one sweep; dy itself stays the residual's gradient
            (a, t, sc, sh, mean, invstd, mult), self._dc = self._dc, None
            conv, bn = self._pwl._parts()
            dz, parts = K.bn_gate_act_bwd_data(dy, t, sc, sh, mult, "none", act="none", save_mean=mean, want_parts=True)
            dt = bn.backward(dz, t, sc, sh, mean, invstd, None, dx_out=t, parts=parts)
            conv.wgrad(a, dt)
            d = conv.dgrad(dt, tuple(a.shape))
        else:
            d = self._pwl.bwd(dy)
        if self._pw is None:
            return self._dw.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=res, need_dx=need_dx)
        d = self._dw.bwd(d)
        return self._pw.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=res, need_dx=need_dx)


class EfficientNet(SgxClassifier):
    _head_path = _finetune_key = "_fc"

    def __init__(self, width_coefficient, depth_coefficient, image_size, dropout_rate, num_classes, batch_norm_momentum=0.99, batch_norm_epsilon=1e-3,
                 drop_connect_rate=0.2, depth_divisor=8, min_depth=None, backbone_mode=False, blocks_args=None):
        super().__init__()
        assert isinstance(blocks_args, list), "blocks_args should be a list"
        assert len(blocks_args) > 0, "block args must be greater than 0"
        self._blocks_args = blocks_args
        self.backbone_mode = backbone_mode
        self.drop_connect_rate = drop_connect_rate
        bn_mom, bn_eps = 1 - batch_norm_momentum, batch_norm_epsilon
        rf = lambda f: round_filters(f, width_coefficient, depth_divisor, min_depth)  # noqa: E731

        out_channels = rf(32)
        need_mult4("EfficientNet", "the stem width", out_channels)
        self._stem_pad = _SamePad("_conv_stem", 3, 2, image_size)
        self._conv_stem = ConvLayer(3, out_channels, 3, 2, 1, bias=False)
        self._bn0 = BatchNorm(out_channels, eps=bn_eps, momentum=bn_mom)
        image_size = calculate_output_image_size(image_size, 2)

        blocks = []
        for block_args in self._blocks_args:
            block_args = block_args._replace(input_filters=rf(block_args.input_filters), output_filters=rf(block_args.output_filters),
                                             num_repeat=round_repeats(block_args.num_repeat, depth_coefficient))
            blocks.append(MBConvBlock(block_args, batch_norm_momentum, batch_norm_epsilon, image_size=image_size, name=f"_blocks.{len(blocks)}"))
            image_size = calculate_output_image_size(image_size, block_args.stride)
            if block_args.num_repeat > 1:  # the repeats keep the output size
                block_args = block_args._replace(input_filters=block_args.output_filters, stride=1)
            for _ in range(block_args.num_repeat - 1):
                blocks.append(MBConvBlock(block_args, batch_norm_momentum, batch_norm_epsilon, image_size=image_size, name=f"_blocks.{len(blocks)}"))
        self._blocks = nn.ModuleList(blocks)

        in_channels = block_args.output_filters
        out_channels = rf(1280)
        need_mult4("EfficientNet", "the head width", out_channels)
        self._conv_head = ConvLayer(in_channels, out_channels, 1, 1, 0, bias=False)
        self._bn1 = BatchNorm(out_channels, eps=bn_eps, momentum=bn_mom)
        self._head_channels = out_channels
        if not self.backbone_mode:
            self._dropout = Dropout(dropout_rate)
            self._fc = LinearLayer(out_channels, num_classes)
        self._stem = ConvBNView(self._conv_stem, self._bn0, "silu")
        self._head = ConvBNView(self._conv_head, self._bn1, "silu")

    # ---- forward / backward --------------------------------------------------------------------------------------
    def _fwd(self, x):
        xh = self._input_nhwc(x)
        self._stem_pad.check(x.shape[2], x.shape[3])
        a = self._stem.fwd(xh)
        nb = len(self._blocks)
        for idx, blk in enumerate(self._blocks):
            rate = self.drop_connect_rate
            if rate:
                rate *= float(idx) / nb
            a = blk.fwd(a, drop_connect_rate=rate)
        a = self._head.fwd(a)
        if self.backbone_mode:
            return (K.nhwc_to_nchw(a),)
        return (self._pool_head_fwd(a, self._fc, self._dropout.p),)

    def _bwd(self, d_out):
        ready = self._bucket_ready
        if self.backbone_mode:
            d = K.nchw_to_nhwc(d_out)
        else:
            d = self._pool_head_bwd(d_out, self._fc)
            ready("_fc.")
        d = self._head.bwd(d)
        ready("_bn1.")
        ready("_conv_head.")
        for i in range(len(self._blocks) - 1, -1, -1):
            d = self._blocks[i].bwd(d)
            ready(f"_blocks.{i}.")
        self._stem.bwd(d, need_dx=False)
        ready("_bn0.")
        ready("_conv_stem.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["_conv_stem.", "_bn0."] + [f"_blocks.{i}." for i in range(len(self._blocks))] + ["_conv_head.", "_bn1.", "_fc."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def replace_input_channels(self, in_channels: int, compute_new_weights_fn=None):
        """Reference :542-545 with modules/weight_replacement_utils.py: the stem keeps the weights of the channels it already has; extra
        channels are drawn from a normal distribution with the old weights' mean / std.  Before materialisation only."""
        if self._materialized:
            raise RuntimeError("replace_input_channels must be called before the model is materialized in HBM (before the first forward)")
        self._conv_stem = widen_conv_input(self._conv_stem, in_channels, compute_new_weights_fn)
        self._stem = ConvBNView(self._conv_stem, self._bn0, "silu")

    def get_input_channels(self) -> int:
        return self._conv_stem.in_channels

    def load_state_dict(self, state_dict: dict, strict: bool = True, **kw):
        """The reference's rule (:550-574): as a backbone, the checkpoint's last two entries (the classifier) are dropped and the 'module.'
        prefix of the remaining names is removed."""
        sd = state_dict.copy()
        if self.backbone_mode:
            sd = OrderedDict(sd)
            sd.popitem()
            sd.popitem()
            sd = OrderedDict((name.split("module.")[1], v) for name, v in sd.items())
        return super().load_state_dict(sd, strict, **kw)


BLOCK_STRINGS = ["r1_k3_s11_e1_i32_o16_se0.25", "r2_k3_s22_e6_i16_o24_se0.25", "r2_k5_s22_e6_i24_o40_se0.25", "r3_k3_s22_e6_i40_o80_se0.25",
                 "r3_k5_s11_e6_i80_o112_se0.25", "r4_k5_s22_e6_i112_o192_se0.25", "r1_k3_s11_e6_i192_o320_se0.25"]


def get_efficientnet_params(width: float, depth: float, res: float, dropout: float, arch_params):
    """The block table (EfficientNet-B0's; the constructor scales it) and the arch params: the variant's defaults overridden by the user's."""
    blocks_args = BlockDecoder.decode(list(BLOCK_STRINGS))
    user = arch_params.to_dict() if isinstance(arch_params, HpmStruct) else dict(arch_params or {})
    user.pop("schema", None)
    new = HpmStruct(width_coefficient=width, depth_coefficient=depth, image_size=res, dropout_rate=dropout, num_classes=get_param(arch_params, "num_classes"),
                    batch_norm_momentum=0.99, batch_norm_epsilon=1e-3, drop_connect_rate=0.2, depth_divisor=8, min_depth=None, backbone_mode=False)
    new.override(**user)
    return blocks_args, new


def _build(self, width, depth, res, dropout, arch_params, num_classes):
    blocks_args, ap = get_efficientnet_params(width, depth, res, dropout, arch_params)
    EfficientNet.__init__(self, blocks_args=blocks_args, num_classes=num_classes or ap.num_classes, backbone_mode=ap.backbone_mode,
                          batch_norm_momentum=ap.batch_norm_momentum, batch_norm_epsilon=ap.batch_norm_epsilon, image_size=ap.image_size,
                          width_coefficient=ap.width_coefficient, depth_divisor=ap.depth_divisor, min_depth=ap.min_depth,
                          depth_coefficient=ap.depth_coefficient, dropout_rate=ap.dropout_rate, drop_connect_rate=ap.drop_connect_rate)


def _variant(name, cls_name, width, depth, res, dropout):
    def init(self, arch_params, num_classes=None):
        _build(self, width, depth, res, dropout, arch_params, num_classes)

    return register_model(name)(type(cls_name, (EfficientNet,), {"__init__": init, "__doc__": f"width {width}, depth {depth}, resolution {res}, dropout {dropout}"}))


EfficientNetB0 = _variant("efficientnet_b0", "EfficientNetB0", 1.0, 1.0, 224, 0.2)
EfficientNetB1 = _variant("efficientnet_b1", "EfficientNetB1", 1.0, 1.1, 240, 0.2)
EfficientNetB2 = _variant("efficientnet_b2", "EfficientNetB2", 1.1, 1.2, 260, 0.3)
EfficientNetB3 = _variant("efficientnet_b3", "EfficientNetB3", 1.2, 1.4, 300, 0.3)
EfficientNetB4 = _variant("efficientnet_b4", "EfficientNetB4", 1.4, 1.8, 380, 0.4)
EfficientNetB5 = _variant("efficientnet_b5", "EfficientNetB5", 1.6, 2.2, 456, 0.4)
EfficientNetB6 = _variant("efficientnet_b6", "EfficientNetB6", 1.8, 2.6, 528, 0.5)
EfficientNetB7 = _variant("efficientnet_b7", "EfficientNetB7", 2.0, 3.1, 600, 0.5)
EfficientNetB8 = _variant("efficientnet_b8", "EfficientNetB8", 2.2, 3.6, 672, 0.5)
EfficientNetL2 = _variant("efficientnet_l2", "EfficientNetL2", 4.3, 5.3, 800, 0.5)


@register_model("CustomizedEfficientnet")
class CustomizedEfficientnet(EfficientNet):
    """width_coefficient, depth_coefficient, res and dropout_rate come from arch_params."""

    def __init__(self, arch_params, num_classes=None):
        g = lambda k: get_param(arch_params, k)  # noqa: E731
        _build(self, g("width_coefficient"), g("depth_coefficient"), g("res"), g("dropout_rate"), arch_params, num_classes)
