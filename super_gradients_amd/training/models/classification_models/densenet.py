"""DenseNet classifiers on the HIP kernels.

Reference: training/models/classification_models/densenet.py - _DenseLayer (:22-45), _DenseBlock (:48-65), _Transition (:68-74), DenseNet
(:77-144), the registered variants (:147-181).  Same constructor arguments, initial weight distributions and state_dict keys
(features.conv0.weight, features.norm0.*, features.denseblock{i}.denselayer{j}.{norm1,conv1,norm2,conv2}.*, features.transition{i}.{norm,conv}.*,
features.norm5.*, classifier.*), so checkpoints interchange both ways.

A dense layer is BatchNorm -> ReLU -> conv1x1 -> BatchNorm -> ReLU -> conv3x3 over the CONCATENATION of everything before it.  Here a block
keeps one concat buffer [N, H, W, C_total]: whatever produces the block's input writes the first slice (the stem's max-pool, a transition's
convolution), every layer reads a channel prefix and its conv3x3 writes growth_rate channels behind that prefix - there is no concat pass.
Two things a translation of the reference would not do:
  * Shared batch statistics.  The batch sums of a channel do not depend on which BatchNorm reads it, so they are folded ONCE, from the
    partial rows the slice's producer leaves (a convolution's epilogue), into the block's statistics record (kernels.dense_record, fp64
    [2][C_total]); every norm1, the transition's norm and norm5 finalise their own scale / shift / running statistics from a prefix of it
    (sgx_dense_bn_finalize).  No statistics sweep re-reads the concat buffer; synchronised BatchNorm is one all-reduce per produced slice.
  * Transition order.  The reference runs norm -> relu -> conv1x1 -> avgpool2x2; convolution and pool are linear and commute, so here it is
    norm -> relu -> avgpool as ONE sweep (sgx_bn_act_avgpool2_fwd: reads the map once, writes a quarter) -> conv1x1 on a quarter of the pixels.
    Results differ from the reference's order by fp32 rounding only.
Per layer (training): norm1 finalize -> z1 = relu(s * prefix + t) (sgx_affine_act_fwd, stored: conv1's weight gradient reads it) -> conv1
(statistics in its epilogue) -> norm2 finalize -> ReLU sweep -> conv3x3 straight into the next slice (statistics into the record)
[-> dropout in place on the slice, its statistics then from sgx_channel_stats_partial].
Backward: one gradient buffer per block, written completely by the block's consumer (the transition's fused backward, or norm5's backward);
layers in reverse - a layer's slice of the buffer is complete when it is reached: conv2 backward, norm2 backward, conv1 backward, then
norm1's backward ADDED into the prefix (sgx_dense_bn_bwd_apply).

Not built (each raises NotImplementedError): growth_rate, num_init_features, bn_size * growth_rate or a transition's halved width that is
not a multiple of 4 (16-byte channel groups); replace_head(new_head=...); half-precision inference.
"""
import torch
from torch import nn

from .... import kernels as K
from ....common.registry import register_model
from ....modules.conv_bn_act_block import ConvBNView
from ....modules.classifier import SgxClassifier, num_classes_of
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, LinearLayer, MaxPool, need_mult4
from ...utils.utils import get_param


class _Record:
    """A block's statistics record and what its readers need to know about it: count = elements per channel behind the sums (all ranks'
    when the BatchNorms are synchronised)."""

    __slots__ = ("sums", "count", "sync")

    def __init__(self, channels, rows, device, sync):
        self.sums = K.dense_record(channels, device)
        self.count, self.sync = rows, sync

    def put(self, parts, c_off, rows):
        world = K.dense_stats_reduce(parts, self.sums, c_off, sync=self.sync)
        self.count = rows * world

    @staticmethod
    def of(x, sync):
        """the record of a tensor nobody left statistics for (a block run on its own)"""
        n, h, w, c = x.shape
        rec = _Record(c, n * h * w, x.device, sync)
        rec.put(K.channel_stats_partial(x), 0, n * h * w)
        return rec


class DenseLayer(SgxBlock):
    """Reference _DenseLayer: norm1, conv1 (1x1), norm2, conv2 (3x3); relu1 / relu2 carry no state."""

    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate):
        super().__init__()
        need_mult4("DenseNet", "a dense layer's input width", num_input_features)
        need_mult4("DenseNet", "growth_rate", growth_rate)
        need_mult4("DenseNet", "bn_size * growth_rate", bn_size * growth_rate)
        self.norm1 = BatchNorm(num_input_features)
        self.conv1 = ConvLayer(num_input_features, bn_size * growth_rate, 1, 1, 0, bias=False)
        self.norm2 = BatchNorm(bn_size * growth_rate)
        self.conv2 = ConvLayer(bn_size * growth_rate, growth_rate, 3, 1, 1, bias=False)
        self.drop_rate = float(drop_rate)
        self.bottleneck = ConvBNView(self.conv1, self.norm2, "relu")  # conv1 -> norm2 -> relu2 (owns no parameter)
        self.cin, self.growth = num_input_features, growth_rate

    def on_materialize(self):
        pass

    def run(self, buf, rec):
        """Read buf[..., :cin], write buf[..., cin : cin + growth]; training: the new slice's sums go into the record."""
        cin, g = self.cin, self.growth
        prefix, new = buf[..., :cin], buf[..., cin:cin + g]
        sc, sh, mean, invstd = self.norm1.scale_shift_record(rec, cin, self.training)
        z1 = K.affine_act(prefix, sc, sh, act="relu")
        a = self.bottleneck.fwd(z1)
        if not self.training:
            self.conv2.conv(a, out=new)
            return
        rows = buf.shape[0] * buf.shape[1] * buf.shape[2]
        seed = None
        if self.drop_rate > 0:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # torch's default generator: torch.manual_seed repeats a step
            self.conv2.conv(a, out=new)
            K.dropout(new, self.drop_rate, seed, out=new)
            parts = K.channel_stats_partial(new)
        else:
            _, parts = self.conv2.conv(a, out=new, stats=True)
        rec.put(parts, cin, rows)
        self._ctx = (sc, sh, mean, invstd, a, seed)

    def back(self, buf, dbuf):
        """dbuf[..., cin : cin + growth] is complete: this layer's input gradient is added to dbuf[..., :cin]."""
        cin, g = self.cin, self.growth
        (sc, sh, mean, invstd, a, seed), self._ctx = self._ctx, None
        prefix, dnew = buf[..., :cin], dbuf[..., cin:cin + g]
        if seed is not None:
            K.dropout(dnew, self.drop_rate, seed, out=dnew)  # the same mask, regenerated
        self.conv2.wgrad(a, dnew)
        da = self.conv2.dgrad(dnew, tuple(a.shape), reqs=[self.bottleneck.bn_reduce_request()])
        # norm1's reduce rows ride in conv1's data gradient where it can carry them
        n1 = self.norm1
        req = K.BnReduceRequest(prefix, sc, sh, mean, "relu") if (self._net.fuse_bn_reduce and not n1._synced()) else None
        dz1 = self.bottleneck.bwd(da, dx_req=[req] if req is not None else None)
        K.dense_bn_bwd(dz1, prefix, sc, sh, n1.weight, mean, invstd, n1.weight.grad, n1.bias.grad, dbuf[..., :cin], act="relu", sync=n1._synced(),
                       parts=req.parts if req is not None else None)

    # ---- on its own (the reference's _DenseLayer(x) -> the new features): a one-layer block
    def fwd(self, x, out=None):
        n, h, w, _ = x.shape
        buf = torch.empty(n, h, w, self.cin + self.growth, device=x.device, dtype=torch.float32)
        K.axpy(x, out=buf[..., :self.cin])
        self._buf = buf if self.training else None
        rec = None
        if self.training:
            rec = _Record(self.cin + self.growth, n * h * w, x.device, self.norm1._synced())
            rec.put(K.channel_stats_partial(buf[..., :self.cin]), 0, n * h * w)
        self.run(buf, rec)
        return buf[..., self.cin:] if out is None else K.axpy(buf[..., self.cin:], out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        buf, self._buf = self._buf, None
        dbuf = torch.zeros(buf.shape, device=dy.device, dtype=torch.float32)
        K.axpy(dy, out=dbuf[..., self.cin:])
        self.back(buf, dbuf)
        return _hand_over(dbuf[..., :self.cin], dx_out, accumulate, addend, need_dx)


def _hand_over(dx, dx_out, accumulate, addend, need_dx):
    """the SgxBlock.bwd protocol for a gradient that already sits in a block's gradient buffer"""
    if not need_dx:
        return None
    if addend is not None:
        K.axpy(addend, out=dx, accumulate=True)
    if dx_out is None:
        return dx
    return K.axpy(dx, out=dx_out, accumulate=accumulate)


class DenseBlock(SgxBlock):
    """Reference _DenseBlock: denselayer1 .. denselayer{num_layers} over one concat buffer."""

    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size, drop_rate))
        self.cin = num_input_features
        self.cout = num_input_features + num_layers * growth_rate

    def on_materialize(self):
        pass

    def layers(self):
        return list(self._modules.values())

    def _synced(self):
        return self.layers()[0].norm1._synced()

    def open(self, n, h, w, device):
        """-> (the concat buffer, its first slice - for the producer of the block's input to write, its record)"""
        buf = torch.empty(n, h, w, self.cout, device=device, dtype=torch.float32)
        rec = _Record(self.cout, n * h * w, device, self._synced()) if self.training else None
        return buf, buf[..., :self.cin], rec

    def run(self, buf, rec):
        """The first slice and its sums are in place: every layer appends its slice -> the buffer."""
        for layer in self.layers():
            layer.run(buf, rec)
        self._buf = buf if self.training else None
        return buf

    def back(self, dbuf):
        """dbuf: the gradient of the whole buffer, written by the block's consumer -> dbuf[..., :cin] is the input gradient afterwards."""
        buf, self._buf = self._buf, None
        for layer in reversed(self.layers()):
            layer.back(buf, dbuf)
        return dbuf[..., :self.cin]

    # ---- on its own (the reference's _DenseBlock(x) -> the concatenation)
    def fwd(self, x, out=None):
        n, h, w, _ = x.shape
        buf, first, rec = self.open(n, h, w, x.device)
        if out is not None:
            buf = out
            first = buf[..., :self.cin]
        K.axpy(x, out=first)
        if rec is not None:
            rec.put(K.channel_stats_partial(first), 0, n * h * w)
        return self.run(buf, rec)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        return _hand_over(self.back(K.axpy(dy)), dx_out, accumulate, addend, need_dx)  # (a copy: the caller's dy is not the block's to add into)


class Transition(SgxBlock):
    """Reference _Transition: norm, relu, conv (1x1), pool (2x2 average) - run as (norm, relu, pool) in one sweep, then conv."""

    def __init__(self, num_input_features, num_output_features):
        super().__init__()
        need_mult4("DenseNet", "a transition's input width", num_input_features)
        need_mult4("DenseNet", "a transition's output width (half its input)", num_output_features)
        self.norm = BatchNorm(num_input_features)
        self.conv = ConvLayer(num_input_features, num_output_features, 1, 1, 0, bias=False)

    def on_materialize(self):
        pass

    def run(self, x, rec, out=None, stats=False):
        """x with its record (None in eval mode) -> conv(pool(relu(norm(x)))) [, the partial rows of its statistics]"""
        sc, sh, mean, invstd = self.norm.scale_shift_record(rec, x.shape[3], self.training)
        p = K.bn_act_avgpool2_fwd(x, sc, sh, act="relu")
        self._ctx = (x, p, sc, sh, mean, invstd) if self.training else None
        return self.conv.conv(p, out=out, stats=stats)

    def back(self, dy, dx_out=None):
        """-> the complete gradient of x (dx_out: the producing block's gradient buffer; every element is written)"""
        (x, p, sc, sh, mean, invstd), self._ctx = self._ctx, None
        self.conv.wgrad(p, dy)
        dp = self.conv.dgrad(dy, tuple(p.shape))
        if dx_out is None:
            dx_out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        n = self.norm
        return K.bn_act_avgpool2_bwd(dp, x, sc, sh, n.weight, mean, invstd, n.weight.grad, n.bias.grad, dx_out, act="relu", sync=n._synced())

    def fwd(self, x, out=None):
        return self.run(x, _Record.of(x, self.norm._synced()) if self.training else None, out=out)

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        if accumulate or addend is not None:
            return _hand_over(self.back(dy), dx_out, accumulate, addend, need_dx)
        return self.back(dy, dx_out)


class _Features(nn.Module):
    """Namespace with the child names of the reference's nn.Sequential `features`."""


class DenseNet(SgxClassifier):
    _head_path = _finetune_key = "classifier"

    def __init__(self, growth_rate: int, structure: list, num_init_features: int, bn_size: int, drop_rate: float, num_classes: int, in_channels: int = 3):
        super().__init__()
        need_mult4("DenseNet", "num_init_features", num_init_features)
        need_mult4("DenseNet", "growth_rate", growth_rate)
        f = self.features = _Features()
        f.add_module("conv0", ConvLayer(in_channels, num_init_features, 7, 2, 3, bias=False))
        f.add_module("norm0", BatchNorm(num_init_features))
        f.add_module("pool0", MaxPool(3, 2, 1))
        self._order = []  # ("block" | "transition", child name) in execution order
        num_features = num_init_features
        for i, num_layers in enumerate(structure):
            f.add_module("denseblock%d" % (i + 1), DenseBlock(num_layers, num_features, bn_size, growth_rate, drop_rate))
            self._order.append(("block", "denseblock%d" % (i + 1)))
            num_features += num_layers * growth_rate
            if i != len(structure) - 1:
                f.add_module("transition%d" % (i + 1), Transition(num_features, num_features // 2))
                self._order.append(("transition", "transition%d" % (i + 1)))
                num_features //= 2
        f.add_module("norm5", BatchNorm(num_features))
        self.num_features = num_features
        self.classifier = LinearLayer(num_features, num_classes)
        self.stem = ConvBNView(f.conv0, f.norm0, "relu")  # conv0 -> norm0 -> relu0 (owns no parameter)
        # reference :121-128 (torchvision's): kaiming-normal convolutions, BatchNorm 1 / 0, zero linear bias
        for m in self.modules():
            if isinstance(m, ConvLayer):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, LinearLayer):
                nn.init.constant_(m.bias, 0)

    def _fwd(self, x):
        f = self.features._modules
        a = self.stem.fwd(self._input_nhwc(x))
        # every block's input is written into the first slice of its concat buffer by its producer, whose statistics open the record
        n, h, w = a.shape[0], (a.shape[1] - 1) // 2 + 1, (a.shape[2] - 1) // 2 + 1  # (the 3x3 / 2 max-pool with padding 1)
        blk = f[self._order[0][1]]
        buf, first, rec = blk.open(n, h, w, a.device)
        f["pool0"].fwd(a, out=first)
        if rec is not None:
            rec.put(K.channel_stats_partial(first), 0, n * h * w)
        for kind, name in self._order:
            if kind == "block":
                blk = f[name]
                buf = blk.run(buf, rec)
                continue
            nxt = f[self._order[self._order.index((kind, name)) + 1][1]]
            n, h, w = buf.shape[0], buf.shape[1] // 2, buf.shape[2] // 2
            nbuf, first, nrec = nxt.open(n, h, w, buf.device)
            if nrec is None:
                f[name].run(buf, None, out=first)
            else:
                _, parts = f[name].run(buf, rec, out=first, stats=True)
                nrec.put(parts, 0, n * h * w)
            buf, rec = nbuf, nrec
        n5 = f["norm5"]
        sc, sh, mean, invstd = n5.scale_shift_record(rec, self.num_features, self.training)
        self._tail = (buf, sc, sh, mean, invstd) if self.training else None
        return (self._pool_head_fwd(K.affine_act(buf, sc, sh, act="relu"), self.classifier),)  # (F.relu, then adaptive_avg_pool2d(1))

    def _bwd(self, d_logits):
        f = self.features._modules
        ready = self._bucket_ready
        (buf, sc, sh, mean, invstd), self._tail = self._tail, None
        d = self._pool_head_bwd(d_logits, self.classifier)
        ready("classifier.")
        # norm5's backward writes the last block's whole gradient buffer
        dbuf = f["norm5"].backward(d, buf, sc, sh, mean, invstd, "relu")
        ready("features.norm5.")
        for kind, name in reversed(self._order):
            if kind == "block":
                d = f[name].back(dbuf)
            else:
                dbuf = f[name].back(d)  # writes the whole gradient buffer of the block before it
            ready(f"features.{name}.")
        d = f["pool0"].bwd(d)
        self.stem.bwd(d, need_dx=False)
        ready("features.norm0.")
        ready("features.conv0.")

    def gradient_buckets(self):
        """Arena ranges in parameter order (GradientAllReducer matches by name prefix)."""
        return ["features.conv0.", "features.norm0."] + [f"features.{name}." for _, name in self._order] + ["features.norm5.", "classifier."]

    # ---- SgModule-style helpers the reference exposes -------------------------------------------------------------
    def get_input_channels(self) -> int:
        return self.features._modules["conv0"].in_channels

    def _new_head(self, new_num_classes):
        super()._new_head(new_num_classes)
        nn.init.constant_(self.classifier.bias, 0)


@register_model("custom_densenet")
class CustomizedDensnet(DenseNet):  # (the reference's spelling)
    def __init__(self, arch_params, num_classes=None):
        super().__init__(growth_rate=get_param(arch_params, "growth_rate", 32), structure=get_param(arch_params, "structure", [6, 12, 24, 16]),
                         num_init_features=get_param(arch_params, "num_init_features", 64), bn_size=get_param(arch_params, "bn_size", 4),
                         drop_rate=get_param(arch_params, "drop_rate", 0), num_classes=num_classes_of(arch_params, num_classes))


def _densenet(name, growth_rate, structure, num_init_features):
    def init(self, arch_params, num_classes=None):
        DenseNet.__init__(self, growth_rate, structure, num_init_features, 4, 0, num_classes_of(arch_params, num_classes))

    return register_model(name)(type(name.replace("densenet", "DenseNet"), (DenseNet,), {"__init__": init}))


DenseNet121 = _densenet("densenet121", 32, [6, 12, 24, 16], 64)
DenseNet161 = _densenet("densenet161", 48, [6, 12, 36, 24], 96)
DenseNet169 = _densenet("densenet169", 32, [6, 12, 32, 32], 64)
DenseNet201 = _densenet("densenet201", 32, [6, 12, 48, 32], 64)
