"""EffectiveSEBlock on the HIP kernels (reference: modules/se_blocks.py:29-42):  y = x * hardsigmoid(project(mean_hw(x))).

Kernels: one deterministic per-image column reduction for the mean ([N,C]), the 1x1 `project` convolution on the [N,1,1,C] means
through the ordinary conv kernels, one gate sweep.  Backward: d(pre) = hardsigmoid'(pre) * sum_hw(dy * x) (one reduction), the
project convolution's weight / data gradients, then dx = dy * gate + d(mean)/HW in one sweep.
"""
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
