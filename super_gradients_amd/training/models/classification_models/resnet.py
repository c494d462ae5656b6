"""ResNet / CifarResNet on the HIP kernels.

Reference: training/models/classification_models/resnet.py - BasicResNetBlock (:26-50), Bottleneck (:53-84), CifarResNet
(:87-137), ResNet (:140-260), the registered variants (:263-375).  Same constructor arguments for the supported subset,
same state_dict keys (conv1.weight, bn1.*, layer{i}.{j}.{conv1,bn1,conv2,bn2[,conv3,bn3]}, layer{i}.{j}.shortcut.{0,1}, linear.*).

Kernel sequence of a block (training):
    t1 = conv1(x)  [BN statistics from the conv epilogue]   a1 = relu(bn1(t1))                 one sweep
    t2 = conv2(a1) ...                                      (bottleneck: one more conv/BN/ReLU)
    shortcut: identity, or ts = conv_s(x) -> u = bn_s(ts)                                       one sweep
    out = relu(bn_last(t_last) + shortcut)                                                      one sweep (affine + residual + act)
Backward: g = dy * [out > 0] (sgx_relu_bwd: the ReLU follows the residual add, so its mask comes from `out`), then the BN
backward sweeps / weight gradients / data gradients of the branch, the shortcut gradient folded into the data-gradient
epilogue (identity) or produced by the shortcut conv's own backward.
"""
from .... import kernels as K
from ....common.registry import register_model
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, LinearLayer, MaxPool, Numbered, widen_conv_input
from ...utils.utils import get_param


def width_multiplier(original, factor, to_int=True):
    return int(original * factor) if to_int else original * factor


class _ConvBN:
    """conv -> training-mode BN bookkeeping shared by the blocks (not a module: the owners register conv/bn themselves)."""

    @staticmethod
    def fwd(conv: ConvLayer, bn: BatchNorm, x, training):
        if training:
            t, parts = conv.conv(x, stats=True)
            M = t.shape[0] * t.shape[1] * t.shape[2]
            return (t,) + tuple(bn.scale_shift(parts, M, True))
        t = conv.conv(x)
        return (t,) + tuple(bn.scale_shift(None, 0, False))


class ResBlock(SgxBlock):
    """out = [relu]( bn_n(conv_n(... relu(bn_1(conv_1(x))) ...)) + shortcut(x) )
    Eval folds: a subclass may set `_folded = {branch index: (filter, bias)}` for layers whose conv has `conv_with` (resnext.py's
    GroupedConvBlock does in prep_model_for_conversion); eval-mode fwd() then runs relu(conv_with(...)) for those layers.  Only layers
    before the last; the attribute name is the one SgxNetwork.weights_changed() clears."""

    _folded = None

    def _branch(self):
        raise NotImplementedError

    def on_materialize(self):
        pass

    def _init_shortcut(self, in_planes, out_planes, stride):
        self.shortcut = Numbered()  # (keys shortcut.0.weight / shortcut.1.*; empty: the identity)
        if stride != 1 or in_planes != out_planes:
            self.shortcut.add_module("0", ConvLayer(in_planes, out_planes, 1, stride, 0, bias=False))
            self.shortcut.add_module("1", BatchNorm(out_planes))

    def _shortcut_fwd(self, x):
        ts, scs, shs, ms, ivs = _ConvBN.fwd(getattr(self.shortcut, "0"), getattr(self.shortcut, "1"), x, self.training)
        return K.affine_act(ts, scs, shs), (ts, scs, shs, ms, ivs)

    def fwd(self, x, out=None):
        branch = self._branch()
        saved = []
        a = x
        # the projection shortcut (conv -> BatchNorm, three short dependent kernels) meets the main branch in its last sweep: branch stream
        # (engine.fork_branch, site 16), joined there
        net = getattr(self, "_net", None)
        forked = None
        self._branched = bool(len(self.shortcut)) and net is not None and self.training and net.branches(16, x.shape[0] * x.shape[1] * x.shape[2], 64)
        if self._branched:
            forked = net.fork_branch(lambda: self._shortcut_fwd(x))
        folded = None if self.training else self._folded
        for i, (conv, bn) in enumerate(branch):
            last = i == len(branch) - 1
            if folded is not None and i in folded and not last:
                a = conv.conv_with(a, folded[i][0], folded[i][1], act="relu")
                saved.append(None)
                continue
            t, sc, sh, mean, invstd = _ConvBN.fwd(conv, bn, a, self.training)
            if not last:
                nxt = K.affine_act(t, sc, sh, act="relu", out=None if self.training else t)
                saved.append((a, t, sc, sh, mean, invstd))
                a = nxt
            else:
                saved.append((a, t, sc, sh, mean, invstd))
        short = x
        sc_ctx = None
        if forked is not None:
            (short, sc_ctx), joined = forked
            joined()
        elif len(self.shortcut):
            short, sc_ctx = self._shortcut_fwd(x)
        _, t, sc, sh, _, _ = saved[-1]
        y = K.affine_act(t, sc, sh, r1=short, a1=1.0, act="relu" if self.final_relu else None, out=out)
        self._ctx = (x, saved, sc_ctx, y) if self.training else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x, saved, sc_ctx, y), self._ctx = self._ctx, None
        branch = self._branch()
        # the final ReLU's mask and the reduce of the last BatchNorm's backward in one sweep (sgx_relu_bwd_bn_reduce, round 6: 16 reduce sweeps
        # of a ResNet-50 step gone); SGX_FUSE_BN_REDUCE=0 or a synchronised BatchNorm: the two passes
        parts_last = None
        if self.final_relu and self._net.fuse_bn_reduce and not branch[-1][1]._synced():
            g, parts_last = K.relu_bwd_bn_reduce(dy, y, saved[-1][1], saved[-1][4])
        else:
            g = K.relu_bwd(dy, y) if self.final_relu else dy
        # the projection shortcut's backward needs g only: forked at the start onto the branch stream (when its forward ran there: its saved
        # tensors are that stream's pool's), its data gradient into a tensor of its own that the main branch's last data gradient adds in its
        # epilogue - the same two-term sum as the accumulate pass
        net = getattr(self, "_net", None)
        fork_sc = (sc_ctx is not None and getattr(self, "_branched", False) and net is not None and net.branches(16, 0, 0, True)
                   and need_dx and addend is None and not accumulate)
        if fork_sc:
            def shortcut_bwd():
                ts, scs, shs, ms, ivs = sc_ctx
                cs, bs = getattr(self.shortcut, "0"), getattr(self.shortcut, "1")
                dts = bs.backward(g, ts, scs, shs, ms, ivs, None, dx_out=ts)
                cs.wgrad(x, dts)
                return cs.dgrad(dts, tuple(x.shape))

            dxs, joined = net.fork_branch(shortcut_bwd, backward=True)
        d = g
        parts = parts_last
        for i in range(len(branch) - 1, 0, -1):
            conv, bn = branch[i]
            a, t, sc, sh, mean, invstd = saved[i]
            dt = bn.backward(d, t, sc, sh, mean, invstd, None if i == len(branch) - 1 else "relu", dx_out=t, parts=parts)
            conv.wgrad(a, dt)
            # (round 6) the BatchNorm-backward reduce of the layer below rides in this data gradient's epilogue (sgx_bn_reduce_req: the launch
            # that writes that layer's output gradient also leaves its two per-channel sums) - as the YOLO-NAS blocks have done since round 4;
            # the ResNet blocks still ran a reduce sweep over (gradient, saved conv output) per layer: 32 of a ResNet-50 step's 53
            _, pt, psc, psh, pmean, _ = saved[i - 1]
            pbn = branch[i - 1][1]
            # (a grouped convolution's data gradient carries no requests: the layer below reduces in its own sweep)
            req = K.BnReduceRequest(pt, psc, psh, pmean, "relu") if (self._net.fuse_bn_reduce and not pbn._synced() and not conv.grouped) else None
            d = conv.dgrad(dt, tuple(a.shape), reqs=[req] if req is not None else None)
            parts = req.parts if req is not None else None
        conv, bn = branch[0]
        a, t, sc, sh, mean, invstd = saved[0]
        dt = bn.backward(d, t, sc, sh, mean, invstd, None if len(branch) == 1 else "relu", dx_out=t, parts=parts)
        conv.wgrad(x, dt)
        if fork_sc:
            joined()
            return conv.dgrad(dt, tuple(x.shape), out=dx_out, addend=dxs)
        if sc_ctx is not None:
            ts, scs, shs, ms, ivs = sc_ctx
            cs, bs = getattr(self.shortcut, "0"), getattr(self.shortcut, "1")
            dts = bs.backward(g, ts, scs, shs, ms, ivs, None, dx_out=ts)
            cs.wgrad(x, dts)
        if not need_dx:
            return None
        shape = tuple(x.shape)
        if sc_ctx is not None:
            dx = conv.dgrad(dt, shape, out=dx_out, accumulate=accumulate, addend=addend)
            return getattr(self.shortcut, "0").dgrad(dts, shape, out=dx, accumulate=True)
        dx = conv.dgrad(dt, shape, out=dx_out, accumulate=accumulate, addend=g)  # identity shortcut: + g in the epilogue
        if addend is not None:
            K.axpy(addend, out=dx, accumulate=True)
        return dx


class BasicResNetBlock(ResBlock):
    def __init__(self, in_planes, planes, stride=1, expansion=1, final_relu=True, droppath_prob=0.0):
        super().__init__()
        if droppath_prob:
            raise NotImplementedError("DropPath (droppath_prob > 0) is not on the HIP path")
        self.expansion, self.final_relu = expansion, final_relu
        self.conv1 = ConvLayer(in_planes, planes, 3, stride, 1, bias=False)
        self.bn1 = BatchNorm(planes)
        self.conv2 = ConvLayer(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = BatchNorm(planes)
        self._init_shortcut(in_planes, expansion * planes, stride)

    def _branch(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]


class Bottleneck(ResBlock):
    def __init__(self, in_planes, planes, stride=1, expansion=4, final_relu=True, droppath_prob=0.0):
        super().__init__()
        if droppath_prob:
            raise NotImplementedError("DropPath (droppath_prob > 0) is not on the HIP path")
        self.expansion, self.final_relu = expansion, final_relu
        self.conv1 = ConvLayer(in_planes, planes, 1, 1, 0, bias=False)
        self.bn1 = BatchNorm(planes)
        self.conv2 = ConvLayer(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = BatchNorm(planes)
        self.conv3 = ConvLayer(planes, expansion * planes, 1, 1, 0, bias=False)
        self.bn3 = BatchNorm(expansion * planes)
        self._init_shortcut(in_planes, expansion * planes, stride)

    def _branch(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]


class ResNetBase(SgxClassifier):
    """Shared driver: stem -> layer1..4 -> global average pool -> linear, and its backward."""

    _head_path = _finetune_key = "linear"  # the classifier's attribute name (ResNeXt: fc)

    def _make_layer(self, block, planes, num_blocks, stride):
        if num_blocks == 0:
            raise NotImplementedError("ResNet layers with num_blocks == 0 (conv-only layers of the customised variants) are not on the HIP path")
        blocks = []
        for s in [stride] + [1] * (num_blocks - 1):
            blocks.append(block(self.in_planes, planes, s, self.expansion) if block is Bottleneck else block(self.in_planes, planes, s, self.expansion))
            self.in_planes = planes * self.expansion
        return Numbered(blocks)  # (keys layer{i}.{j}.*)

    def _stem_fwd(self, xh):
        raise NotImplementedError

    def _stem_bwd(self, d):
        raise NotImplementedError

    def _fwd(self, x):
        a = self._stem_fwd(self._input_nhwc(x))
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer.blocks():
                a = blk.fwd(a)
        return (self._pool_head_fwd(a, getattr(self, self._head_path)),)

    def _bwd(self, d_logits):
        d = self._pool_head_bwd(d_logits, getattr(self, self._head_path))
        ready = self._bucket_ready
        ready(f"{self._head_path}.")
        for name in ("layer4", "layer3", "layer2", "layer1"):
            for blk in reversed(getattr(self, name).blocks()):
                d = blk.bwd(d)
            ready(f"{name}.")
        self._stem_bwd(d)
        ready("bn1.")
        ready("conv1.")

    def gradient_buckets(self):
        """Arena ranges in parameter order; `stem` covers conv1/bn1 (GradientAllReducer matches by name prefix)."""
        return ["conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.", f"{self._head_path}."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.conv1.in_channels

    def replace_input_channels(self, in_channels: int, compute_new_weights_fn=None):
        """Reference resnet.py:130-136, 249-258 with modules/weight_replacement_utils.py:24-65: conv1 keeps the weights of the channels it
        already has; extra channels are drawn from a normal distribution with the old weights' mean / std.  Before materialisation only."""
        if self._materialized:
            raise RuntimeError("replace_input_channels must be called before the model is materialized in HBM (before the first forward)")
        self.conv1 = widen_conv_input(self.conv1, in_channels, compute_new_weights_fn)


class CifarResNet(ResNetBase):
    def __init__(self, block, num_blocks, num_classes=10, width_mult=1, expansion=1, in_channels: int = 3):
        super().__init__()
        self.expansion = expansion
        self.structure = [num_blocks, width_mult]
        self.in_planes = width_multiplier(64, width_mult)
        self.conv1 = ConvLayer(in_channels, width_multiplier(64, width_mult), 3, 1, 1, bias=False)
        self.bn1 = BatchNorm(width_multiplier(64, width_mult))
        self.layer1 = self._make_layer(block, width_multiplier(64, width_mult), num_blocks[0], 1)
        self.layer2 = self._make_layer(block, width_multiplier(128, width_mult), num_blocks[1], 2)
        self.layer3 = self._make_layer(block, width_multiplier(256, width_mult), num_blocks[2], 2)
        self.layer4 = self._make_layer(block, width_multiplier(512, width_mult), num_blocks[3], 2)
        self.linear = LinearLayer(width_multiplier(512, width_mult) * expansion, num_classes)

    def _stem_fwd(self, xh):
        t, sc, sh, mean, invstd = _ConvBN.fwd(self.conv1, self.bn1, xh, self.training)
        a = K.affine_act(t, sc, sh, act="relu", out=None if self.training else t)
        self._stem = (xh, t, sc, sh, mean, invstd) if self.training else None
        return a

    def _stem_bwd(self, d):
        (xh, t, sc, sh, mean, invstd), self._stem = self._stem, None
        dt = self.bn1.backward(d, t, sc, sh, mean, invstd, "relu", dx_out=t)
        self.conv1.wgrad(xh, dt)


class ResNet(ResNetBase):
    def __init__(self, block, num_blocks: list, num_classes: int = 10, width_mult: float = 1, expansion: int = 1, droppath_prob=0.0,
                 input_batchnorm: bool = False, backbone_mode: bool = False, in_channels: int = 3):
        super().__init__()
        if droppath_prob or input_batchnorm or backbone_mode:
            raise NotImplementedError("ResNet on the HIP path: droppath_prob=0, input_batchnorm=False, backbone_mode=False")
        self.expansion, self.width_mult = expansion, width_mult
        self.structure = [num_blocks, width_mult]
        self.in_planes = width_multiplier(64, width_mult)
        self.conv1 = ConvLayer(in_channels, width_multiplier(64, width_mult), 7, 2, 3, bias=False)
        self.bn1 = BatchNorm(width_multiplier(64, width_mult))
        self.maxpool = MaxPool(3, 2, 1)
        self.layer1 = self._make_layer(block, width_multiplier(64, width_mult), num_blocks[0], 1)
        self.layer2 = self._make_layer(block, width_multiplier(128, width_mult), num_blocks[1], 2)
        self.layer3 = self._make_layer(block, width_multiplier(256, width_mult), num_blocks[2], 2)
        self.layer4 = self._make_layer(block, width_multiplier(512, width_mult), num_blocks[3], 2)
        self.linear = LinearLayer(width_multiplier(512, width_mult) * expansion, num_classes)

    def _stem_fwd(self, xh):
        t, sc, sh, mean, invstd = _ConvBN.fwd(self.conv1, self.bn1, xh, self.training)
        a = K.affine_act(t, sc, sh, act="relu", out=None if self.training else t)
        self._stem = (xh, t, sc, sh, mean, invstd) if self.training else None
        return self.maxpool.fwd(a)

    def _stem_bwd(self, d):
        (xh, t, sc, sh, mean, invstd), self._stem = self._stem, None
        d = self.maxpool.bwd(d)
        dt = self.bn1.backward(d, t, sc, sh, mean, invstd, "relu", dx_out=t)
        self.conv1.wgrad(xh, dt)


def _resnet(name, block, layers, expansion=1):
    def init(self, arch_params, num_classes=None):
        ResNet.__init__(self, block, layers, num_classes=num_classes_of(arch_params, num_classes), expansion=expansion,
                        droppath_prob=get_param(arch_params, "droppath_prob", 0), backbone_mode=get_param(arch_params, "backbone_mode", False))

    return register_model(name)(type(name.title().replace("_", ""), (ResNet,), {"__init__": init}))


ResNet18 = _resnet("resnet18", BasicResNetBlock, [2, 2, 2, 2])
ResNet34 = _resnet("resnet34", BasicResNetBlock, [3, 4, 6, 3])
ResNet50 = _resnet("resnet50", Bottleneck, [3, 4, 6, 3], expansion=4)
ResNet101 = _resnet("resnet101", Bottleneck, [3, 4, 23, 3], expansion=4)
ResNet152 = _resnet("resnet152", Bottleneck, [3, 8, 36, 3], expansion=4)


@register_model("resnet18_cifar")
class ResNet18Cifar(CifarResNet):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(BasicResNetBlock, [2, 2, 2, 2], num_classes=num_classes_of(arch_params, num_classes))


@register_model("resnet50_3343")
class ResNet50_3343(ResNet):
    def __init__(self, arch_params, num_classes=None):
        super().__init__(Bottleneck, [3, 3, 4, 3], num_classes=num_classes_of(arch_params, num_classes), expansion=4,
                         droppath_prob=get_param(arch_params, "droppath_prob", 0), backbone_mode=get_param(arch_params, "backbone_mode", False))
