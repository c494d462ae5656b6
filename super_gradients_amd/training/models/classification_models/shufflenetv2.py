"""ShuffleNetV2 classifiers on the HIP kernels.

Reference: training/models/classification_models/shufflenetv2.py - ChannelShuffleInvertedResidual (:24-112), ShuffleNetV2Base (:115-210), the
registered variants (:213-242).  Same constructor arguments, default PyTorch initialisation and state_dict keys (conv1.{0,1}.*,
layer{2,3,4}.{i}.branch1.{0,1,2,3}.* (stride-2 blocks only), layer{2,3,4}.{i}.branch2.{0,1,3,4,5,6}.*, conv5.{0,1}.*, fc.*), so checkpoints
interchange both ways.

The block is `chunk -> branch -> cat -> channel_shuffle(2)`.  The reference pays a full-width read and write for the cat, another for the
shuffle's transpose().contiguous(), and autograd the same again backwards.  Here none of them is a pass: the sweep that applies branch2's last
BatchNorm -> ReLU anyway (sgx_shuffle_merge_fwd) also carries the other half and stores both, interleaved, as the block's output; the next
stride-1 block's chunk is two channel-slice views of that buffer.  Backward, the last BatchNorm's reduce and apply sweeps load the interleaved
gradient and take it apart in registers (sgx_shuffle_merge_bwd_reduce / _bwd_apply); the pass-through half's gradient is stored by the apply
sweep into the left channel slice of the block's input gradient, the first 1x1 convolution's data gradient fills the right slice.

Per block (training):
  stride 1: conv1x1 on x[..., h:] (statistics in its epilogue) -> bn_finalize -> affine + ReLU sweep -> depthwise 3x3 -> bn_finalize -> affine
            sweep -> conv1x1 -> bn_finalize -> merge sweep (left: x[..., :h] copied, right: affine + ReLU).
  stride 2: the same branch2 on all of x with the depthwise layer at stride 2; branch1: depthwise 3x3 / 2 -> bn_finalize -> affine sweep ->
            conv1x1 -> bn_finalize; merge sweep with an affine + ReLU side each.  The two branches run one after the other on the main stream.
Backward: merge reduce (one sweep, both BatchNorms' rows at stride 2) -> each BatchNorm's finalize -> merge apply (in place over the saved
conv outputs) -> per branch: weight gradient (side stream), data gradient, layer by layer as MobileNetV2's InvertedResidual.  At stride 2
branch2's first data gradient writes dx and branch1's depthwise data gradient accumulates into it.
Eval: the merge with the running statistics' scale / shift; after prep_model_for_conversion() the folded convolutions carry bias + ReLU in
their epilogues and the merge runs with two copy sides.

The 16-byte contract decides which variants run.  Every sweep and convolution entry point needs channel counts, slice offsets and row strides
that are multiples of 4 floats, so a block's HALF width must be a multiple of 4: x0_5 (24 / 48 / 96), x1_5 (88 / 176 / 352) and custom models
whose stage widths are multiples of 8.  Stage 2 of shufflenet_v2_x1_0 has half width 58 and of shufflenet_v2_x2_0 122 (both = 2 mod 4: the
x[..., h:] slice would start at an 8-byte address): both names are registered and raise NotImplementedError at construction.  No channel is
padded behind the parameters' backs.

Not built (each raises NotImplementedError where reachable): backbone_mode=True; block stride 3; x1_0 / x2_0 (above);
replace_head(new_head=...); half-precision inference.
"""
import torch

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNSeq, ConvBNView
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, DepthwiseConvLayer, LinearLayer, MaxPool, Numbered, need_mult4
from ...utils.utils import get_param


_WHY_MULT4 = "every sweep and convolution moves 16-byte channel groups, and the block's halves are channel slices that must start on one"


class ChannelShuffleInvertedResidual(SgxBlock):
    """Reference ChannelShuffleInvertedResidual: branch1.{0,1,2,3} (stride 2 only), branch2.{0,1,3,4,5,6}; ReLUs carry no state."""

    def __init__(self, inp: int, out: int, stride: int):
        super().__init__()
        assert 1 <= stride <= 3, "Illegal stride value"
        assert (stride != 1) or (inp == out), "When stride == 1 num of input channels should be equal to the requested num of out output channels"
        if stride == 3:
            raise NotImplementedError("ShuffleNetV2 on the HIP path: block stride 1 or 2 (the depthwise kernels have no stride 3)")
        h = out // 2
        need_mult4("ShuffleNetV2", f"the half width of a block ({inp} -> {out} channels)", h, why=_WHY_MULT4)
        need_mult4("ShuffleNetV2", "a stride-2 block's input width", inp if stride > 1 else 0, why=_WHY_MULT4)
        if out != 2 * h:
            raise NotImplementedError(f"ShuffleNetV2 on the HIP path: an even block width, got {out}")
        self.stride, self.h = stride, h
        if stride > 1:
            b1 = {"0": DepthwiseConvLayer(inp, stride), "1": BatchNorm(inp), "2": ConvLayer(inp, h, 1, 1, 0), "3": BatchNorm(h)}
            self.branch1 = Numbered(**b1)
        else:
            self.branch1 = None  # (the reference's nn.Identity: no state)
        b2 = {"0": ConvLayer(inp if stride > 1 else inp // 2, h, 1, 1, 0), "1": BatchNorm(h), "3": DepthwiseConvLayer(h, stride), "4": BatchNorm(h),
              "5": ConvLayer(h, h, 1, 1, 0), "6": BatchNorm(h)}
        self.branch2 = Numbered(**b2)
        # the conv -> BatchNorm (-> ReLU) sequences over those layers (they own no parameter: nothing is added to the state); the last one of
        # a branch stops before its affine sweep (fwd_raw): the merge sweep is that sweep
        self.pw = ConvBNView(b2["0"], b2["1"], "relu")
        self.dw = ConvBNView(b2["3"], b2["4"], None)
        self.pwl = ConvBNView(b2["5"], b2["6"], "relu")
        self.dw1 = ConvBNView(b1["0"], b1["1"], None) if stride > 1 else None
        self.pwl1 = ConvBNView(b1["2"], b1["3"], "relu") if stride > 1 else None

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        h = self.h
        if self.stride == 1:
            if x.shape[3] != 2 * h:
                raise ValueError(f"a stride-1 block of width {2 * h} got {x.shape[3]} channels")
            left, lraw = x[..., :h], (None,) * 5  # (the chunk: two channel-slice views)
            a = self.pw.fwd(x[..., h:])
        else:
            lraw = self.pwl1.fwd_raw(self.dw1.fwd(x))
            left = lraw[0]
            a = self.pw.fwd(x)
        rraw = self.pwl.fwd_raw(self.dw.fwd(a))
        y = K.shuffle_merge(left, rraw[0], lscale=lraw[1], lshift=lraw[2], lact="relu" if lraw[1] is not None else None,
                            rscale=rraw[1], rshift=rraw[2], ract="relu" if rraw[1] is not None else None, out=out)
        self._ctx = (tuple(x.shape), lraw, rraw) if self.training else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x_shape, lraw, rraw), self._ctx = self._ctx, None
        bn2 = self.branch2._modules["6"]
        right = (rraw[0], rraw[1], rraw[2], rraw[3], rraw[4], "relu", bn2)
        if self.stride == 1:
            # the apply sweep writes dx[..., :h] (the pass-through half's gradient, bit for bit), branch2's first data gradient dx[..., h:]
            h = self.h
            own = dx_out is None or accumulate
            dx = torch.empty(x_shape, device=dy.device, dtype=torch.float32) if own else dx_out
            K.shuffle_merge_bwd(dy, dx[..., :h], right)
            d = self.dw.bwd(self.pwl.bwd_from_dt(rraw[0]))
            self.pw.bwd(d, dx_out=dx[..., h:])
            if not need_dx:
                return None
            if addend is not None:
                K.axpy(addend, out=dx, accumulate=True)
            if own and dx_out is not None:
                return K.axpy(dx, out=dx_out, accumulate=True)
            return dx
        bn1 = self.branch1._modules["3"]
        K.shuffle_merge_bwd(dy, (lraw[0], lraw[1], lraw[2], lraw[3], lraw[4], "relu", bn1), right)
        d = self.dw.bwd(self.pwl.bwd_from_dt(rraw[0]))
        dx = self.pw.bwd(d, dx_out=dx_out, accumulate=accumulate, addend=addend, need_dx=need_dx)
        d1 = self.pwl1.bwd_from_dt(lraw[0])
        self.dw1.bwd(d1, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class ShuffleNetV2Base(SgxClassifier):
    _head_path = _finetune_key = "fc"

    def __init__(self, structure, stages_out_channels, backbone_mode: bool = False, num_classes: int = 1000, block=ChannelShuffleInvertedResidual,
                 in_channels: int = 3):
        super().__init__()
        if backbone_mode:
            raise NotImplementedError("ShuffleNetV2 on the HIP path: backbone_mode=False (ShuffleNet as a detection backbone is not built)")
        if len(structure) != 3:
            raise ValueError("expected structure as list of 3 positive ints")
        if len(stages_out_channels) != 5:
            raise ValueError("expected stages_out_channels as list of 5 positive ints")
        self.backbone_mode = backbone_mode
        self.structure = structure
        self.out_channels = stages_out_channels
        c = self.out_channels
        need_mult4("ShuffleNetV2", "the stem's width", c[0], why=_WHY_MULT4)
        self.conv1 = ConvBNSeq(in_channels, c[0], 3, stride=2, padding=1, activation_type="relu")
        self.maxpool = MaxPool(3, 2, 1)
        self.layer2 = self._make_layer(block, c[0], c[1], structure[0])
        self.layer3 = self._make_layer(block, c[1], c[2], structure[1])
        self.layer4 = self._make_layer(block, c[2], c[3], structure[2])
        need_mult4("ShuffleNetV2", "conv5's width", c[4], why=_WHY_MULT4)
        self.conv5 = ConvBNSeq(c[3], c[4], 1, stride=1, padding=0, activation_type="relu")
        self.fc = LinearLayer(c[4], num_classes)

    @staticmethod
    def _make_layer(block, input_channels, output_channels, repeats):
        seq = [block(input_channels, output_channels, 2)] + [block(output_channels, output_channels, 1) for _ in range(repeats - 1)]
        return Numbered(seq)

    def _fwd(self, x):
        a = self.maxpool.fwd(self.conv1.fwd(self._input_nhwc(x)))
        for layer in (self.layer2, self.layer3, self.layer4):
            for blk in layer.blocks():
                a = blk.fwd(a)
        return (self._pool_head_fwd(self.conv5.fwd(a), self.fc),)

    def _bwd(self, d_logits):
        ready = self._bucket_ready
        d = self._pool_head_bwd(d_logits, self.fc)
        ready("fc.")
        d = self.conv5.bwd(d)
        ready("conv5.")
        for name in ("layer4", "layer3", "layer2"):
            for blk in reversed(getattr(self, name).blocks()):
                d = blk.bwd(d)
            ready(f"{name}.")
        self.conv1.bwd(self.maxpool.bwd(d), need_dx=False)
        ready("conv1.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["conv1.", "layer2.", "layer3.", "layer4.", "conv5.", "fc."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.conv1._modules["0"].in_channels


def _shufflenet(name, cls_name, stages_out_channels):
    def init(self, arch_params, num_classes: int = None, backbone_mode: bool = False):
        ShuffleNetV2Base.__init__(self, [4, 8, 4], stages_out_channels, backbone_mode=backbone_mode, num_classes=num_classes_of(arch_params, num_classes))

    return register_model(name)(type(cls_name, (ShuffleNetV2Base,), {"__init__": init}))


ShufflenetV2_x0_5 = _shufflenet("shufflenet_v2_x0_5", "ShufflenetV2_x0_5", [24, 48, 96, 192, 1024])
ShufflenetV2_x1_0 = _shufflenet("shufflenet_v2_x1_0", "ShufflenetV2_x1_0", [24, 116, 232, 464, 1024])  # (half width 58: refuses, see above)
ShufflenetV2_x1_5 = _shufflenet("shufflenet_v2_x1_5", "ShufflenetV2_x1_5", [24, 176, 352, 704, 1024])
ShufflenetV2_x2_0 = _shufflenet("shufflenet_v2_x2_0", "ShufflenetV2_x2_0", [24, 244, 488, 976, 2048])  # (half width 122: refuses)


@register_model("shufflenet_v2_custom5")
class CustomizedShuffleNetV2(ShuffleNetV2Base):
    def __init__(self, arch_params, num_classes: int = None, backbone_mode: bool = False):
        super().__init__(get_param(arch_params, "structure"), get_param(arch_params, "stages_out_channels"), backbone_mode=backbone_mode,
                         num_classes=num_classes_of(arch_params, num_classes))
