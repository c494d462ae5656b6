"""EffectiveSEBlock on the HIP kernels (reference: modules/se_blocks.py:29-42):  y = x * hardsigmoid(project(mean_hw(x))).

Kernels: one deterministic per-image column reduction for the mean ([N,C]), the 1x1 `project` convolution on the [N,1,1,C] means
through the ordinary conv kernels, one gate sweep.  Backward: d(pre) = hardsigmoid'(pre) * sum_hw(dy * x) (one reduction), the
project convolution's weight / data gradients, then dx = dy * gate + d(mean)/HW in one sweep.
"""
from math import sqrt

import torch
from torch import nn

from .. import kernels as K
from .engine import SgxBlock
from .layers import ConvLayer, LinearLayer


class EffectiveSEBlock(SgxBlock):
    GATE = "hardsigmoid"

    def __init__(self, in_channels: int):
        super().__init__()
        self.project = ConvLayer(in_channels, in_channels, 1, 1, 0, bias=True)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        n, h, w, c = x.shape
        mean = K.image_colsum(x, scale=1.0 / (h * w)).view(n, 1, 1, c)
        pre = self.project.conv(mean).view(n, c)
        self._ctx = (x, mean, pre) if self.training else None
        return K.channel_gate(x, pre, self.GATE, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, mean, pre), self._ctx = self._ctx, None
        n, h, w, c = x.shape
        dpre = K.image_colsum(dy, v=x, pre=pre, gate=self.GATE).view(n, 1, 1, c)
        self.project.wgrad(mean, dpre)
        dmean = self.project.dgrad(dpre, (n, 1, 1, c)).view(n, c)
        if addend is not None:
            raise NotImplementedError("EffectiveSEBlock.bwd: no addend")
        if dx_out is None:
            dx_out, accumulate = dy, False  # in place over the incoming gradient (element-wise: each value is read before it is written)
        return K.channel_gate(dy, pre, self.GATE, bias=dmean, bias_scale=1.0 / (h * w), out=dx_out, accumulate=accumulate)


def _make_divisible(v, divisor, min_value=None):
    """The reference's rounding rule (classification_models/mobilenetv3.py:18-31)."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class _Fc(SgxBlock):
    """Namespace with the numeric child names of the reference's nn.Sequential (fc.0, fc.2; 1 and 3 are ReLU and h_sigmoid: no state)."""

    def on_materialize(self):
        pass


class SELayer(SgxBlock):
    """MobileNetV3's SELayer (classification_models/mobilenetv3.py:52-67): y = x * h_sigmoid(fc(mean_hw(x))), fc = Linear -> ReLU -> Linear;
    keys fc.0.*, fc.2.*.  h_sigmoid is the hard-sigmoid gate.  Used in two positions:
      after the activation (fwd / bwd): image_colsum -> fc -> channel_gate, like EffectiveSEBlock;
      between a BatchNorm and its activation (fwd_fused / bwd_fused, called by ConvBNView(gate=...)): the BatchNorm output z is never stored -
      its per-image means are the affine map of the convolution output's means, and one sweep computes act(gate * z); backward: one reduction
      for d(pre), then one sweep that writes dz and the BatchNorm backward's reduce rows."""

    GATE = "hardsigmoid"
    after_act = False  # ConvBNView(gate=self): act(gate * bn)

    def __init__(self, channel: int, reduction: int = 4):
        super().__init__()
        hidden = _make_divisible(channel // reduction, 8)
        self.channel, self.hidden = channel, hidden
        self.fc = _Fc()
        self.fc.add_module("0", LinearLayer(channel, hidden))
        self.fc.add_module("2", LinearLayer(hidden, channel))

    def on_materialize(self):
        pass

    def _mlp(self, m):
        n = m.shape[0]
        h = self.fc._modules["0"].fwd(m).contiguous()
        hr = K.affine_act(h.view(n, 1, 1, self.hidden), act="relu")
        self._hr = hr if self.training else None
        return self.fc._modules["2"].fwd(hr.view(n, self.hidden)).contiguous()

    def _mlp_bwd(self, dpre):
        hr, self._hr = self._hr, None
        n = dpre.shape[0]
        dh = self.fc._modules["2"].bwd(dpre).contiguous()
        dh = K.relu_bwd(dh.view(n, 1, 1, self.hidden), hr, out=dh.view(n, 1, 1, self.hidden))
        return self.fc._modules["0"].bwd(dh.view(n, self.hidden)).contiguous()

    # ---- after the activation
    def fwd(self, x, out=None):
        n, h, w, c = x.shape
        pre = self._mlp(K.image_colsum(x, scale=1.0 / (h * w)))
        self._ctx = (x, pre) if self.training else None
        return K.channel_gate(x, pre, self.GATE, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, pre), self._ctx = self._ctx, None
        n, h, w, c = x.shape
        if addend is not None:
            raise NotImplementedError("SELayer.bwd: no addend")
        dmean = self._mlp_bwd(K.image_colsum(dy, v=x, pre=pre, gate=self.GATE))
        if dx_out is None:
            dx_out, accumulate = dy, False  # in place over the incoming gradient (element-wise)
        return K.channel_gate(dy, pre, self.GATE, bias=dmean, bias_scale=1.0 / (h * w), out=dx_out, accumulate=accumulate)

    # ---- between BatchNorm and activation: t is the convolution output, z = scale * t + shift (None: z = t)
    def fwd_fused(self, t, scale, shift, act, out=None):
        n, h, w, c = t.shape
        m = K.image_colsum(t, scale=1.0 / (h * w))
        if scale is not None:
            m = K.affine_act(m.view(n, 1, 1, c), scale, shift).view(n, c)  # the means of z: an [N,C] matrix, not a pass over the map
        pre = self._mlp(m)
        self._pre = pre if self.training else None
        return K.bn_gate_act_fwd(t, scale, shift, pre, self.GATE, act=act, out=out)

    def bwd_fused(self, dy, t, scale, shift, save_mean, act):
        """-> (dz, reduce rows of (dz, t) for the BatchNorm backward); dz is written over dy"""
        pre, self._pre = self._pre, None
        dmean = self._mlp_bwd(K.bn_gate_act_bwd_gate(dy, t, scale, shift, pre, self.GATE, act=act))
        return K.bn_gate_act_bwd_data(dy, t, scale, shift, pre, self.GATE, act=act, dmean=dmean, save_mean=save_mean, out=dy, want_parts=True)


class _SEConv(SgxBlock):
    """Parameters of one of an SE branch's nn.Conv2d(cin, cout, 1, bias=True): weight [cout, cin, 1, 1], bias [cout]."""

    def __init__(self, cin, cout):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, 1
        self.weight = nn.Parameter(torch.empty(cout, cin, 1, 1))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.kaiming_uniform_(self.weight, a=sqrt(5))
        nn.init.uniform_(self.bias, -1.0 / sqrt(cin), 1.0 / sqrt(cin))

    def on_materialize(self):
        pass


class ConvSqueezeExcite(SgxBlock):
    """x * sigmoid(conv2(act(conv1(mean_hw(x))))) with two nn.Conv2d(..., 1, bias=True) whose parameters keep the reference's shapes.  The
    hidden width is often no multiple of 4 (4 is, 6, 10, 22, 38, 94 are not): it is padded to the next one inside with zero filter rows / bias
    in the first convolution and zero columns in the second; the padded gradients are dropped.  Subclasses say where the two _SEConv live
    (`_convs`) and which activation sits between them (ACT: relu - RegNet's SqueezeExcite; silu - EfficientNet's MBConvSE).
    Two positions, as SELayer has them:
      after the activation, on a stored map (fwd / bwd): image_colsum -> the two convolutions on [N,1,1,C] -> channel_gate;
      after_act = True, called by ConvBNView(gate=...) (fwd_fused / bwd_fused): BatchNorm -> activation -> gate on the sgx_bn_act_gate_*
      sweeps - the activated map is never stored: one pass for its per-image means, one for y = s * act(z); backward: one reduction for
      d(pre), then one sweep that writes dz and the BatchNorm backward's reduce rows."""

    GATE = "sigmoid"
    ACT = "relu"
    after_act = False  # the order ConvBNView(gate=self) runs: False - act(gate * bn) (SELayer), True - gate * act(bn)
    _folded = None  # eval-mode cache of the zero-padded filters (dropped like the conv + BatchNorm folds)

    def __init__(self, channels, hidden):
        super().__init__()
        if hidden < 1:
            raise ValueError(f"SE hidden width {hidden}: the block's input width is smaller than se_ratio")
        self.channels, self.hidden, self._hp = channels, hidden, (hidden + 3) // 4 * 4

    def on_materialize(self):
        pass

    def _convs(self):
        raise NotImplementedError

    def _filters(self):
        """(w1 [hp, C, 1, 1], b1 [hp], w2 [C, hp, 1, 1]): the parameters themselves, or zero-padded copies when hidden % 4 != 0"""
        c1, c2 = self._convs()
        if self._hp == self.hidden:
            return c1.weight, c1.bias, c2.weight
        if not self.training and self._folded is not None:
            return self._folded
        dev = c1.weight.device
        w1 = torch.zeros(self._hp, self.channels, 1, 1, device=dev)
        w1[: self.hidden].copy_(c1.weight.detach())
        b1 = torch.zeros(self._hp, device=dev)
        b1[: self.hidden].copy_(c1.bias.detach())
        w2 = torch.zeros(self.channels, self._hp, 1, 1, device=dev)
        w2[:, : self.hidden].copy_(c2.weight.detach())
        if not self.training:  # eval: the padded copies are kept until the weights change (train(), SgxNetwork.weights_changed)
            self._folded = (w1, b1, w2)
        return w1, b1, w2

    def train(self, mode: bool = True):
        if mode:
            self._folded = None
        return super().train(mode)

    def _mlp(self, m):
        """per-image means [N,1,1,C] -> the gate's pre-activations [N,C]"""
        n, c = m.shape[0], self.channels
        w1, b1, w2 = self._filters()
        if self.ACT == "relu":  # its backward needs the activated value only: activation in the convolution's epilogue
            h, hr = None, K.conv2d_fwd(m, w1, bias=b1, act="relu")
        else:
            h = K.conv2d_fwd(m, w1, bias=b1)
            hr = K.affine_act(h, act=self.ACT)
        pre = K.conv2d_fwd(hr, w2, bias=self._convs()[1].bias).view(n, c)
        self._mctx = (m, h, hr, w1, w2) if self.training else None
        return pre

    def _mlp_bwd(self, dpre):
        """d(pre) [N,C] -> d(means) [N,C]; the two convolutions' parameter gradients are accumulated"""
        (m, h, hr, w1, w2), self._mctx = self._mctx, None
        n, c = dpre.shape
        c1, c2 = self._convs()
        padded = self._hp != self.hidden
        dpre = dpre.view(n, 1, 1, c)
        gw2 = torch.zeros_like(w2) if padded else c2.weight.grad
        K.conv2d_bwd_weight(hr, dpre, gw2, c2.bias.grad)
        dh = K.conv2d_bwd_data(dpre, w2, (n, 1, 1, self._hp))
        if self.ACT == "relu":
            dh = K.relu_bwd(dh, hr, out=dh)
        else:  # dh * act'(h): the gate sweep's data gradient with a unit gate and no BatchNorm affine
            dh = K.bn_gate_act_bwd_data(dh, h, None, None, torch.ones(n, self._hp, device=dh.device), "none", act=self.ACT, out=dh)
        gw1 = torch.zeros_like(w1) if padded else c1.weight.grad
        gb1 = torch.zeros(self._hp, device=dh.device) if padded else c1.bias.grad
        K.conv2d_bwd_weight(m, dh, gw1, gb1)
        if padded:  # the padded rows / columns saw zero filters: their gradients are dropped, the rest joins the parameters' gradients
            c2.weight.grad.add_(gw2[:, : self.hidden])
            c1.weight.grad.add_(gw1[: self.hidden])
            c1.bias.grad.add_(gb1[: self.hidden])
        return K.conv2d_bwd_data(dh, w1, (n, 1, 1, c)).view(n, c)

    # ---- after the activation, on a stored map
    def fwd(self, x, out=None):
        n, h, w, c = x.shape
        pre = self._mlp(K.image_colsum(x, scale=1.0 / (h * w)).view(n, 1, 1, c))
        self._ctx = (x, pre) if self.training else None
        return K.channel_gate(x, pre, self.GATE, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, pre), self._ctx = self._ctx, None
        if addend is not None:
            raise NotImplementedError(f"{type(self).__name__}.bwd: no addend")
        n, h, w, c = x.shape
        dmean = self._mlp_bwd(K.image_colsum(dy, v=x, pre=pre, gate=self.GATE))
        if dx_out is None:
            dx_out, accumulate = dy, False  # in place over the incoming gradient (element-wise)
        return K.channel_gate(dy, pre, self.GATE, bias=dmean, bias_scale=1.0 / (h * w), out=dx_out, accumulate=accumulate)

    # ---- BatchNorm -> activation -> gate: t is the convolution output, z = scale * t + shift (None: z = t)
    def fwd_fused(self, t, scale, shift, act, out=None):
        n, h, w, c = t.shape
        pre = self._mlp(K.bn_act_gate_mean(t, scale, shift, act=act).view(n, 1, 1, c))
        self._pre = pre if self.training else None
        return K.bn_act_gate_fwd(t, scale, shift, pre, self.GATE, act=act, out=out)

    def bwd_fused(self, dy, t, scale, shift, save_mean, act):
        """-> (dz, reduce rows of (dz, t) for the BatchNorm backward); dz is written over dy"""
        pre, self._pre = self._pre, None
        dmean = self._mlp_bwd(K.bn_act_gate_bwd_gate(dy, t, scale, shift, pre, self.GATE, act=act))
        return K.bn_act_gate_bwd_data(dy, t, scale, shift, pre, self.GATE, act=act, dmean=dmean, save_mean=save_mean, out=dy, want_parts=True)


class MBConvSE(ConvSqueezeExcite):
    """EfficientNet's squeeze-and-excitation (efficientnet.py:341-346, 375-380): sigmoid(_se_expand(silu(_se_reduce(mean_hw(a))))) * a with
    a = silu(bn1(dw(x))) - after the activation, so ConvBNView(gate=self) runs the sgx_bn_act_gate_* sweeps.  The two convolutions are
    registered by the MBConvBlock under the reference's names (_se_reduce, _se_expand); this object holds them unregistered."""

    ACT = "silu"
    after_act = True

    def __init__(self, reduce_conv, expand_conv):
        super().__init__(reduce_conv.in_channels, reduce_conv.out_channels)
        self._pair = (reduce_conv, expand_conv)  # (a tuple: not registered as sub-modules)

    def _convs(self):
        return self._pair
