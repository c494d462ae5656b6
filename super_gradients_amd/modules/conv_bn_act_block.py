"""conv -> BatchNorm -> activation blocks on the HIP kernels.

Reference classes mirrored (same constructor arguments for the supported subset, same state_dict keys):
  Conv        modules/conv_bn_act_block.py:80-93    keys conv.weight, bn.*       (autopad, no conv bias)
  ConvBNAct   modules/conv_bn_act_block.py:9-69     keys seq.conv.*, seq.bn.*
  ConvBNReLU  modules/conv_bn_relu_block.py:8-60    keys seq.conv.*, seq.bn.*
Kernel sequence (training):  conv (BN partial statistics emitted by the conv epilogue) -> bn_finalize (tiny)
-> affine+activation sweep.  Backward: BN(+act) backward in three sweeps (activation mask recomputed from the saved
conv output, nothing else stored) -> weight gradient -> data gradient.
"""
import torch
from torch import nn

from .. import kernels as K
from .engine import SgxBlock
from .layers import GROUPED_CG, BatchNorm, ConvLayer, DepthwiseConvLayer, GroupedConvLayer, act_name


def _conv_layer(in_channels, out_channels, kernel_size, stride, padding, groups):
    """groups == 1: the implicit-GEMM ConvLayer; groups == in == out with a 3x3 pad-1 or 5x5 pad-2 filter: the depthwise layer; 1 < groups < in == out
    with a 3x3 pad-1 filter and 4, 8, 16, 32 or 64 channels per group: the grouped layer; anything else raises."""
    if groups in (None, 1):
        return ConvLayer(in_channels, out_channels, kernel_size, stride, padding, bias=False)
    if groups == in_channels == out_channels and (kernel_size, padding) in ((3, 1), (5, 2)):
        return DepthwiseConvLayer(in_channels, stride, kernel_size)
    if (1 < groups < in_channels and in_channels == out_channels and (kernel_size, padding) == (3, 1) and in_channels % groups == 0
            and in_channels // groups in GROUPED_CG and stride in (1, 2)):
        return GroupedConvLayer(in_channels, groups, stride)
    raise NotImplementedError(f"grouped convolution on the HIP path: groups=1, depthwise 3x3 pad 1 / 5x5 pad 2 (groups == in_channels == out_channels), or 3x3 pad 1 "
                              f"stride 1 / 2 with in_channels == out_channels and in_channels / groups in {GROUPED_CG}; got groups={groups}, "
                              f"{in_channels} -> {out_channels}, kernel {kernel_size}, stride {stride}, padding {padding}")


class _ConvBN(SgxBlock):
    """Shared implementation; subclasses only choose where `conv`/`bn` are registered (key names)."""

    _folded = None  # (filter with the BatchNorm scale folded in, shift as bias): eval form set by prep_model_for_conversion
    _gate = None  # (SE object,) fused with the BatchNorm and the activation (ConvBNView(gate=...)): the block then runs on the SE object's sweeps
    _folded_half = None  # the same for a channel-padded filter (C % 4 != 0: an RGB stem) - read by the half-precision path only, which re-lays filters out itself

    def _parts(self):
        raise NotImplementedError

    def on_materialize(self):
        pass

    def prep_model_for_conversion(self, input_size=None, **kwargs):
        """Eval form as ONE launch: act(conv(x, w * s[k]) + t[k]) with s = gamma / sqrt(running_var + eps), t = beta - running_mean * s -
        bias and activation live in the conv epilogue, the BatchNorm apply sweep and the scale/shift kernel of the eval path disappear.
        What torch.nn.utils.fusion.fuse_conv_bn_eval does for the reference's export paths; here the parameters stay as they are (the block
        still trains: train() drops the folded copy), only eval-mode forward reads the folded filter.  One-off preparation in torch ops."""
        conv, bn = self._parts()
        w = conv._w
        if w is None:
            raise RuntimeError("prep_model_for_conversion needs a materialised model (the fold reads the arena views)")
        if conv.depthwise:  # act(dwconv(x, w * s[c]) + t[c]): bias and activation (ReLU6 included) live in the depthwise epilogue
            with torch.no_grad():
                s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
                wf = K.dw_empty(w.shape[0], w.device, w.shape[2])
                wf.copy_(w.detach() * s.view(-1, 1, 1, 1))
                self._folded = (wf, (bn.bias.detach() - bn.running_mean * s).contiguous())
            return
        K_, C_, R_, S_ = w.shape
        if w.stride() != (R_ * S_ * C_, 1, S_ * C_, C_):
            # channel-padded filters (C % 4 != 0): the fp32 path keeps the general eval sequence; the half-precision path converts filters to
            # its own bf16 layout anyway (kernels.half_filter takes any strides) - fold for it alone (prep used to return silently
            # and the bf16 forward then raised "call prep_model_for_conversion() first")
            with torch.no_grad():
                s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
                self._folded_half = ((w.detach() * s.view(-1, 1, 1, 1)).contiguous(), (bn.bias.detach() - bn.running_mean * s).contiguous())
            return
        with torch.no_grad():
            s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
            wf = K.ohwi_empty(K_, C_, R_, S_, w.device)
            wf.copy_(w.detach() * s.view(-1, 1, 1, 1))
            self._folded = (wf, (bn.bias.detach() - bn.running_mean * s).contiguous())

    def train(self, mode: bool = True):
        if mode:
            self._folded = self._folded_half = None  # the weights are about to change
        return super().train(mode)

    def fwd(self, x, out=None, post_add=None, post_scale=None, residual=None):
        """post_add: tensor added AFTER the activation (pp_yolo_head.py:205 `stem_cls(feat, avg_feat) + feat`); its gradient is the
        caller's (dy reaches it unchanged).  post_scale (half-precision inference only): a multiplier of post_add.
        residual (layers without activation only - MobileNetV2's linear bottleneck, mobilenetv2.py:95-97 `x + conv(x)`): added by the
        BatchNorm's own affine sweep (r1 of sgx_affine_act_fwd), not by a pass of its own; its gradient is the caller's too."""
        conv, bn = self._parts()
        if residual is not None:
            if self.act is not None or post_add is not None or x.dtype == K.HALF:
                raise RuntimeError("residual rides in the affine sweep of a layer without activation (fp32)")
        gate = self._gate[0] if self._gate is not None else None
        if gate is not None and (residual is not None or post_add is not None or x.dtype == K.HALF):
            raise RuntimeError("a gate between BatchNorm and activation: fp32, no residual, no post_add")
        if x.dtype == K.HALF:  # half-precision inference: the folded deployment form, everything in ONE bf16 launch
            folded = self._folded if self._folded is not None else self._folded_half
            if self.training or folded is None:
                raise RuntimeError("half-precision inference runs the folded deployment form: call prep_model_for_conversion() in eval mode first")
            if conv.grouped:
                raise NotImplementedError("the grouped convolution has no half-precision kernel")
            return K.conv2d_fwd(x, folded[0], bias=folded[1], out=out, act=self.act, stride=conv.stride, pad=conv.padding,
                                post_add=post_add, post_scale=post_scale)
        if post_scale is not None:
            raise RuntimeError("post_scale: half-precision inference only")
        if self.training:
            self._folded = self._folded_half = None  # a training step follows: a folded eval filter would be stale afterwards
            t, parts = conv.conv(x, stats=True)
            M = t.shape[0] * t.shape[1] * t.shape[2]
            scale, shift, mean, invstd = bn.scale_shift(parts, M, True)
            if gate is not None:
                y = gate.fwd_fused(t, scale, shift, self.act, out=out)
            elif post_add is None:
                y = K.affine_act(t, scale, shift, r1=residual, act=self.act, out=out)
            else:
                y = K.tri_affine_act(t, scale, shift, post_add=post_add, act=self.act, out=out)
            self._ctx = (x, t, scale, shift, mean, invstd)
            self._req = None
            return y
        if gate is not None:  # eval: dwconv + bias (folded) or the plain convolution, then the gate sweep with / without the BatchNorm affine
            if self._folded is not None and (conv.depthwise or conv.grouped):
                t = conv.conv_with(x, self._folded[0], self._folded[1])
                return gate.fwd_fused(t, None, None, self.act, out=out if out is not None else t)
            t = conv.conv(x)
            scale, shift, _, _ = bn.scale_shift(None, 0, False)
            return gate.fwd_fused(t, scale, shift, self.act, out=out if out is not None else t)
        if self._folded is not None and post_add is None:
            if conv.depthwise and residual is None:
                return conv.conv_with(x, self._folded[0], self._folded[1], out=out, act=self.act)
            if conv.grouped:  # act(gconv(x, w) + bias) in one launch; ReLU6 / hard-swish and a residual take the sweep after it
                own = self.act not in ("relu6", "hswish") and residual is None
                t = conv.conv_with(x, self._folded[0], self._folded[1], out=out if own else None, act=self.act if own else None)
                return t if own else K.affine_act(t, r1=residual, act=self.act, out=out if out is not None else t)
            if self.act in ("relu6", "hswish"):  # the conv epilogues do not carry ReLU6 / hard-swish: conv + bias, then the sweep in place
                t = K.conv2d_fwd(x, self._folded[0], bias=self._folded[1], stride=conv.stride, pad=conv.padding)
                return K.affine_act(t, act=self.act, out=out if out is not None else t)
            if not conv.depthwise:
                return K.conv2d_fwd(x, self._folded[0], bias=self._folded[1], addend=residual, out=out, act=self.act, stride=conv.stride, pad=conv.padding)
        t = conv.conv(x)
        scale, shift, _, _ = bn.scale_shift(None, 0, False)
        if post_add is not None:
            return K.tri_affine_act(t, scale, shift, post_add=post_add, act=self.act, out=out if out is not None else t)
        return K.affine_act(t, scale, shift, r1=residual, act=self.act, out=out if out is not None else t)

    def fwd_raw(self, x):
        """The layer WITHOUT its affine + activation sweep, for a caller whose own sweep applies them (ShuffleNetV2's merge,
        shufflenetv2.py): -> (t, scale, shift, save_mean, save_invstd) with y = act(scale * t + shift).  Eval mode: the running statistics'
        scale / shift and no mean / invstd; after prep_model_for_conversion() t is the finished output (bias and activation in the
        convolution's epilogue) and scale / shift are None.  Training keeps what bwd_from_dt() needs."""
        conv, bn = self._parts()
        if self._gate is not None or x.dtype == K.HALF or conv.depthwise or conv.grouped or self.act in ("relu6", "hswish"):
            raise NotImplementedError("fwd_raw: a plain fp32 convolution -> BatchNorm [-> ReLU / SiLU] layer")
        if self.training:
            self._folded = self._folded_half = None
            t, parts = conv.conv(x, stats=True)
            scale, shift, mean, invstd = bn.scale_shift(parts, t.shape[0] * t.shape[1] * t.shape[2], True)
            self._ctx = (x, t, scale, shift, mean, invstd)
            self._req = None
            return t, scale, shift, mean, invstd
        if self._folded is not None:
            y = K.conv2d_fwd(x, self._folded[0], bias=self._folded[1], act=self.act, stride=conv.stride, pad=conv.padding)
            return y, None, None, None, None
        scale, shift, _, _ = bn.scale_shift(None, 0, False)
        return conv.conv(x), scale, shift, None, None

    def bwd_from_dt(self, dt, dx_out=None, accumulate=False, need_dx=True):
        """The rest of the backward of a fwd_raw() step once the caller's sweeps have run the BatchNorm backward (dgamma / dbeta included):
        dt is the gradient of the convolution's output."""
        conv, _ = self._parts()
        (x, _, _, _, _, _), self._ctx = self._ctx, None
        conv.wgrad(x, dt, bias_grad=False)
        if not need_dx:
            return None
        return conv.dgrad(dt, tuple(x.shape), out=dx_out, accumulate=accumulate)

    def bn_reduce_request(self):
        """This layer's BatchNorm-backward reduce as a request for the data-gradient launch that finalises its output gradient (the caller
        hands it to that launch; bwd() then finds the partial sums ready and skips its own reduce sweep).  None when it cannot be handed over
        (synchronised BatchNorm reduces across ranks on its own path)."""
        conv, bn = self._parts()
        if self._ctx is None or bn._synced() or not self._net.fuse_bn_reduce or self.act in ("relu6", "hswish") or self._gate is not None:
            # (the data-gradient epilogues carry neither ReLU6 nor hard-swish nor a gate)
            return None
        _, t, scale, shift, mean, _ = self._ctx
        self._req = K.BnReduceRequest(t, scale, shift, mean, self.act)
        return self._req

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True, dx_req=None):
        """dx_req: reduce requests of the layer(s) whose output gradient is this call's dx (ConvLayer.dgrad)"""
        conv, bn = self._parts()
        (x, t, scale, shift, mean, invstd), self._ctx = self._ctx, None
        req, self._req = getattr(self, "_req", None), None
        parts = req.parts if req is not None else None
        if self._gate is not None:  # dz and the BatchNorm-backward reduce rows from the gate's data-gradient sweep (in place over dy)
            dz, parts = self._gate[0].bwd_fused(dy, t, scale, shift, mean, self.act)
            dt = bn.backward(dz, t, scale, shift, mean, invstd, None, dx_out=t, parts=parts)
        else:
            dt = bn.backward(dy, t, scale, shift, mean, invstd, self.act, dx_out=t, parts=parts)  # in place over the saved conv output
        conv.wgrad(x, dt)
        if not need_dx:
            return None
        return conv.dgrad(dt, tuple(x.shape), out=dx_out, accumulate=accumulate, addend=addend, reqs=dx_req)


class Conv(_ConvBN):
    """Reference `Conv` (conv_bn_act_block.py:80): Conv2d(k, stride, autopad, bias=False) + BatchNorm2d + activation."""

    def __init__(self, input_channels, output_channels, kernel, stride, activation_type, padding: int = None, groups: int = None):
        super().__init__()
        pad = kernel // 2 if padding is None else padding
        self.conv = _conv_layer(input_channels, output_channels, kernel, stride, pad, groups)
        self.bn = BatchNorm(output_channels)
        self.act = act_name(activation_type)

    def _parts(self):
        return self.conv, self.bn


class _Seq(nn.Module):
    """Namespace module so that keys read seq.conv.weight / seq.bn.* like the reference's nn.Sequential."""


class ConvBNAct(_ConvBN):
    """Reference `ConvBNAct` (conv_bn_act_block.py:9-69), supported subset: groups as `_conv_layer` routes them (1, depthwise, grouped 3x3), dilation=1, zero padding, use_normalization=True."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, activation_type=None, stride=1, dilation=1, groups=1, bias=True,
                 padding_mode="zeros", use_normalization=True, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True,
                 device=None, dtype=None, activation_kwargs=None):
        super().__init__()
        if dilation != 1 or padding_mode != "zeros" or not use_normalization or not affine or not track_running_stats:
            raise NotImplementedError("ConvBNAct on the HIP path supports dilation=1, zero padding, affine BN with running stats")
        if bias:
            raise NotImplementedError("conv bias followed by BatchNorm is redundant; the HIP path implements bias=False (as all hot-path call sites use)")
        self.seq = _Seq()
        self.seq.add_module("conv", _conv_layer(in_channels, out_channels, kernel_size, stride, padding, groups))
        self.seq.add_module("bn", BatchNorm(out_channels, eps=eps, momentum=momentum))
        self.act = act_name(activation_type)

    def _parts(self):
        return self.seq.conv, self.seq.bn


class ConvBNSeq(_ConvBN):
    """nn.Sequential(nn.Conv2d(bias=False), nn.BatchNorm2d[, activation]) with the reference's numeric keys 0.weight, 1.* (mobilenetv2.py:39-44
    conv_bn / conv_1x1_bn)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation_type=None, groups=1):
        super().__init__()
        self.add_module("0", _conv_layer(in_channels, out_channels, kernel_size, stride, padding, groups))
        self.add_module("1", BatchNorm(out_channels))
        self.act = act_name(activation_type)

    def _parts(self):
        return self._modules["0"], self._modules["1"]


class ConvBNView(_ConvBN):
    """conv -> BatchNorm -> activation over layers that are registered ELSEWHERE (the numbered entries of a reference nn.Sequential that holds
    several such triples: InvertedResidual.conv, mobilenetv2.py:70-93).  Owns no parameter: it adds nothing to the state_dict."""

    def __init__(self, conv, bn, activation_type=None, gate=None):
        """gate: an SE object (registered elsewhere too) whose fwd_fused / bwd_fused run the BatchNorm, the activation and the gate.  The
        object chooses the order: SELayer (after_act False) sits between the BatchNorm and the activation - y = act(se(bn(conv(x)))), the
        sgx_bn_gate_act_* sweeps; MBConvSE (after_act True) sits after the activation - y = se(act(bn(conv(x)))), the sgx_bn_act_gate_* sweeps."""
        super().__init__()
        self._pair = (conv, bn)  # (a tuple: not registered as sub-modules)
        self.act = act_name(activation_type)
        self._gate = (gate,) if gate is not None else None

    def _parts(self):
        return self._pair


class ConvBNReLU(ConvBNAct):
    """Reference `ConvBNReLU` (conv_bn_relu_block.py:8-60)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, padding_mode="zeros",
                 use_normalization=True, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None,
                 use_activation=True, inplace=False):
        super().__init__(in_channels, out_channels, kernel_size, padding=padding, activation_type="relu" if use_activation else None, stride=stride,
                         dilation=dilation, groups=groups, bias=bias, padding_mode=padding_mode, use_normalization=use_normalization, eps=eps,
                         momentum=momentum, affine=affine, track_running_stats=track_running_stats)
