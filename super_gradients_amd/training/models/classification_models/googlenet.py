"""GoogLeNet (Inception v1) classifier on the HIP kernels.

Reference: training/models/classification_models/googlenet.py - GoogLeNet (:18-166), Inception (:169-193), BasicConv2d (:224-235), the
registered GoogleNetV1 (:238-241).  Same constructor arguments and state_dict keys (conv{1,2,3}.{conv,bn}.*, inception{3a..5b}.branch1.{conv,bn}.*,
.branch{2,3}.{0,1}.{conv,bn}.*, .branch4.1.{conv,bn}.*, fc.*), BatchNorm eps 0.001, so checkpoints interchange both ways.  Initialisation is
torch.nn.init.trunc_normal_(std=0.01, a=-0.02, b=0.02) on every convolution and the linear layer: the law of the reference's
scipy.stats.truncnorm(-2, 2, scale=0.01) draw, not its draws.

The Inception block is four branches over one input, concatenated.  Here a block owns ONE output buffer [N, H, W, C_total]; the last
BatchNorm -> ReLU sweep of every branch writes its channel slice (the offsets are multiples of 4 for every configuration of the reference),
so there is no concat pass; backward reads dy slice by slice, the first branch's data gradient writes dx and the other three accumulate.
Branch 4, MaxPool2d(3, 1, 1) -> conv1x1, runs the fused kernels of csrc/inception.h: the pooled map, its arg-max map and the pooled map's
gradient - each as wide as the block's input - are never stored; the backward recomputes the arg-max from the block's input, which the other
branches keep anyway.  The three 1x1 convolutions that share the input stay three launches.
The three down-sampling pools are ceil_mode=True (sgx_maxpool_ceil_fwd / _bwd).

Not built (each raises NotImplementedError): aux_logits=True (the two auxiliary classifiers), backbone_mode=True, replace_head(new_head=...),
half-precision inference.  The registered googlenet_v1 sets none of them.
"""
import torch

from .... import kernels as K
from ....common.registry import register_model
from ....modules.classifier import SgxClassifier
from ....modules.conv_bn_act_block import _ConvBN
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, Dropout, LinearLayer, MaxPool, Numbered, need_mult4
from ...utils.utils import get_param


class PoolProjLayer(SgxBlock):
    """nn.Conv2d(Ci, Co, 1, bias=False) behind MaxPool2d(3, 1, 1), as the three fused kernels, with ConvLayer's interface.  `pooled` tells
    the owning conv -> BatchNorm block that the folded eval form goes through conv_with() and that there is no half-precision kernel.  The
    data gradient recomputes the arg-max from x: wgrad(), which the owner calls first, keeps it for dgrad(); BasicConv2d.bwd drops it."""

    _param_kinds = {"weight": "conv"}
    depthwise = False
    grouped = False
    pooled = True

    def __init__(self, in_channels, out_channels):
        super().__init__()
        need_mult4("GoogLeNet", "the pool projection's input width", in_channels)
        need_mult4("GoogLeNet", "the pool projection's output width", out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = 1, 1, 0
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels, 1, 1))
        self.register_parameter("bias", None)
        self._w = self._gw = self._x = None

    def on_materialize(self):
        slots = {s.param: s for s in self._net.slots}
        s = slots[self.weight]
        self._w, self._gw = s.kernel_view, s.grad_kernel_view

    def conv(self, x, out=None, act=None, addend=None, stats=False):
        if addend is not None:
            raise NotImplementedError("the pool projection has no pre-activation addend")
        return K.pool3_conv1x1_fwd(x, self._w, out=out, act=act, stat_partials=stats)

    def conv_with(self, x, w, bias, out=None, act=None):
        return K.pool3_conv1x1_fwd(x, w, bias=bias, out=out, act=act)

    def wgrad(self, x, dy, bias_grad=True):
        self._x = x
        self._net.fork_side(lambda: K.pool3_conv1x1_bwd_weight(x, dy, self._gw), x, dy)

    def dgrad(self, dy, x_shape, out=None, accumulate=False, addend=None, reqs=None):
        x, self._x = self._x, None
        if reqs:
            raise NotImplementedError("the pool projection's data gradient carries no BatchNorm-reduce requests")
        if addend is not None:
            if accumulate:
                K.axpy(addend, out=out, accumulate=True)
            else:
                out = K.axpy(addend, out=out)
            accumulate = True
        return K.pool3_conv1x1_bwd_data(dy, self._w, x, out=out, accumulate=accumulate)


class BasicConv2d(_ConvBN):
    """Reference BasicConv2d: conv (bias=False), bn (eps 0.001), relu.  pool3=True: the convolution reads max_pool2d(x, 3, 1, 1)."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, pool3=False):
        super().__init__()
        need_mult4("GoogLeNet", "a convolution's output width", out_channels)
        self.conv = PoolProjLayer(in_channels, out_channels) if pool3 else ConvLayer(in_channels, out_channels, kernel_size, stride, padding, bias=False)
        self.bn = BatchNorm(out_channels, eps=0.001)
        self.act = "relu"

    def _parts(self):
        return self.conv, self.bn

    def bwd(self, dy, **kwargs):
        try:
            return super().bwd(dy, **kwargs)
        finally:
            if getattr(self.conv, "pooled", False):
                self.conv._x = None  # (need_dx=False: no dgrad() took it)


class Inception(SgxBlock):
    """Reference Inception: branch1, branch2.{0,1}, branch3.{0,1}, branch4.1 (branch4.0 is the stateless max-pool, fused into branch4.1)."""

    def __init__(self, in_channels, ch1x1, ch3x3red, ch3x3, ch5x5red, ch5x5, pool_proj, conv_block=None):
        super().__init__()
        if conv_block is not None:
            raise NotImplementedError("Inception on the HIP path: conv_block=None (BasicConv2d)")
        self.branch1 = BasicConv2d(in_channels, ch1x1)
        self.branch2 = Numbered([BasicConv2d(in_channels, ch3x3red), BasicConv2d(ch3x3red, ch3x3, 3, padding=1)])
        self.branch3 = Numbered([BasicConv2d(in_channels, ch5x5red), BasicConv2d(ch5x5red, ch5x5, 3, padding=1)])
        self.branch4 = Numbered(**{"1": BasicConv2d(in_channels, pool_proj, pool3=True)})
        self.widths = (ch1x1, ch3x3, ch5x5, pool_proj)
        self.cout = sum(self.widths)

    def on_materialize(self):
        pass

    def _slices(self, t):
        out, o = [], 0
        for c in self.widths:
            out.append(t[..., o:o + c])
            o += c
        return out

    def fwd(self, x, out=None):
        n, h, w, _ = x.shape
        if out is None:
            out = torch.empty(n, h, w, self.cout, device=x.device, dtype=torch.float32)
        o1, o2, o3, o4 = self._slices(out)
        self.branch1.fwd(x, out=o1)
        for br, o in ((self.branch2, o2), (self.branch3, o3)):
            red, conv = br.blocks()
            conv.fwd(red.fwd(x), out=o)
        self.branch4._modules["1"].fwd(x, out=o4)
        return out

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        d1, d2, d3, d4 = self._slices(dy)
        dx = self.branch1.bwd(d1, dx_out=dx_out, accumulate=accumulate, addend=addend, need_dx=need_dx)
        for br, d in ((self.branch2, d2), (self.branch3, d3)):
            red, conv = br.blocks()
            red.bwd(conv.bwd(d), dx_out=dx, accumulate=True, need_dx=need_dx)
        self.branch4._modules["1"].bwd(d4, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


_STAGES = (("inception3a", (192, 64, 96, 128, 16, 32, 32)), ("inception3b", (256, 128, 128, 192, 32, 96, 64)), ("maxpool3", (3, 2)),
           ("inception4a", (480, 192, 96, 208, 16, 48, 64)), ("inception4b", (512, 160, 112, 224, 24, 64, 64)),
           ("inception4c", (512, 128, 128, 256, 24, 64, 64)), ("inception4d", (512, 112, 144, 288, 32, 64, 64)),
           ("inception4e", (528, 256, 160, 320, 32, 128, 128)), ("maxpool4", (2, 2)),
           ("inception5a", (832, 256, 160, 320, 32, 128, 128)), ("inception5b", (832, 384, 192, 384, 48, 128, 128)))


class GoogLeNet(SgxClassifier):
    _head_path = _finetune_key = "fc"

    def __init__(self, num_classes=1000, aux_logits=True, init_weights=True, backbone_mode=False, dropout=0.3):
        super().__init__()
        if aux_logits:
            raise NotImplementedError("GoogLeNet on the HIP path: aux_logits=False (the auxiliary classifiers are not built)")
        if backbone_mode:
            raise NotImplementedError("GoogLeNet on the HIP path: backbone_mode=False")
        self.num_classes, self.backbone_mode, self.aux_logits, self.dropout_p = num_classes, backbone_mode, aux_logits, dropout
        self.conv1 = BasicConv2d(3, 64, 7, stride=2, padding=3)
        self.maxpool1 = MaxPool(3, 2, 0, ceil_mode=True)
        self.conv2 = BasicConv2d(64, 64, 1)
        self.conv3 = BasicConv2d(64, 192, 3, padding=1)
        self.maxpool2 = MaxPool(3, 2, 0, ceil_mode=True)
        for name, args in _STAGES:
            self.add_module(name, MaxPool(args[0], args[1], 0, ceil_mode=True) if name.startswith("maxpool") else Inception(*args))
        self.aux1 = self.aux2 = None
        self.dropout = Dropout(dropout)
        self.fc = LinearLayer(1024, num_classes)
        self._order = ["conv1", "maxpool1", "conv2", "conv3", "maxpool2"] + [name for name, _ in _STAGES]
        if init_weights:
            self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, (ConvLayer, PoolProjLayer, LinearLayer)):
                torch.nn.init.trunc_normal_(m.weight, mean=0.0, std=0.01, a=-0.02, b=0.02)
            elif isinstance(m, BatchNorm):
                torch.nn.init.constant_(m.weight, 1)
                torch.nn.init.constant_(m.bias, 0)

    def _fwd(self, x):
        a = self._input_nhwc(x)
        for name in self._order:
            a = self._modules[name].fwd(a)
        return (self._pool_head_fwd(a, self.fc, self.dropout.p),)

    def _bwd(self, d_logits):
        ready = self._bucket_ready
        d = self._pool_head_bwd(d_logits, self.fc)
        ready("fc.")
        for name in reversed(self._order[1:]):
            d = self._modules[name].bwd(d)
            if not name.startswith("maxpool"):
                ready(f"{name}.")
        self.conv1.bwd(d, need_dx=False)
        ready("conv1.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return [f"{name}." for name in self._order if not name.startswith("maxpool")] + ["fc."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.conv1.conv.in_channels

    def _new_head(self, new_num_classes):
        super()._new_head(new_num_classes)
        self.num_classes = new_num_classes


@register_model("googlenet_v1")
class GoogleNetV1(GoogLeNet):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(aux_logits=False, num_classes=num_classes or get_param(arch_params, "num_classes"), dropout=get_param(arch_params, "dropout", 0.3))
