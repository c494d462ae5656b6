"""DDRNet's DAPPM context module on the HIP kernels.

Reference: training/models/segmentation_models/ddrnet.py - DAPPMBranch (:44-105), DAPPM (:108-137).  Same constructor arguments and state_dict
keys (branches.{i}.down_scale.{0,2} for the stride-1 branch, .{1,3} behind a pool, branches.{i}.process.{0,2}, compression.{0,2},
shortcut.{0,2}), so checkpoints interchange both ways.  The DDRNet networks around it are not assembled yet: no model name is registered.

Kernel sequence of a forward (training; five branches, csrc/dappm.h):
    sgx_dappm_pool_fwd        ONE launch: the three window pools, the global pool, and the BatchNorm moments of x and of every pooled map
    per BatchNorm             bn_finalize from those partial rows (x's rows serve branch 0's and the shortcut's) -> affine + ReLU sweep -> 1x1 conv
    per pooled branch         sgx_resize_bilinear_fwd: resize to H x W + the previous branch's output + the moments of the sum, one launch
                              -> bn_finalize -> affine + ReLU sweep -> 3x3 conv writing its channel slice of the concat buffer (no concat pass)
    compression, shortcut     the concat buffer's statistics come from the convolutions' epilogues (a DenseNet record); the shortcut's 1x1
                              convolution takes the compression's output as its addend: the module's sum costs no pass.
Backward mirrors it; sgx_dappm_pool_bwd gathers the four pooled gradients and adds the two gradients that reach x directly, writing dx once.

Not built (NotImplementedError at construction): interpolation modes other than "bilinear"; pools outside the pyramid kernel's limits (more than
three window levels, stride above 8, kernel above 17 or below twice the stride); a first branch that pools, or a later one that does not.
"""
import torch

from .... import kernels as K
from ....modules.engine import SgxBlock
from ....modules.layers import BatchNorm, ConvLayer, Numbered, StatsRecord, need_mult4


class _BNReLUConv(SgxBlock):
    """The reference's nn.Sequential([pool,] BatchNorm2d, ReLU, Conv2d(bias=False)): children named by their position in it."""

    def __init__(self, first, in_channels, out_channels, kernel_size):
        super().__init__()
        self.add_module(str(first), BatchNorm(in_channels))
        self.add_module(str(first + 2), ConvLayer(in_channels, out_channels, kernel_size, 1, kernel_size // 2, bias=False))
        self._names = (str(first), str(first + 2))

    def on_materialize(self):
        pass

    def _parts(self):
        return self._modules[self._names[0]], self._modules[self._names[1]]

    def run(self, t, parts=None, rows=0, rec=None, out=None, addend=None, stats=False):
        """conv(relu(bn(t))); the BatchNorm's batch statistics arrive as partial rows over `rows` elements or as a record of the concat buffer."""
        bn, conv = self._parts()
        if rec is not None:
            sc, sh, mean, invstd = bn.scale_shift_record(rec, t.shape[3], self.training)
        else:
            sc, sh, mean, invstd = bn.scale_shift(parts, rows, self.training)
        a = K.affine_act(t, sc, sh, act="relu")
        self._ctx = (t, a, sc, sh, mean, invstd) if self.training else None
        return conv.conv(a, out=out, addend=addend, stats=stats)

    def back(self, du):
        """-> the gradient at t; the parameter gradients are accumulated"""
        (t, a, sc, sh, mean, invstd), self._ctx = self._ctx, None
        bn, conv = self._parts()
        conv.wgrad(a, du)
        return bn.backward(conv.dgrad(du, tuple(a.shape)), t, sc, sh, mean, invstd, "relu")


def _check_pool(kernel_size, stride):
    if not (2 <= stride <= 8 and 2 * stride <= kernel_size <= 17):
        raise NotImplementedError(f"DAPPM on the HIP path: AvgPool2d(kernel {kernel_size}, stride {stride}, padding {stride}) is outside the pyramid "
                                  "kernel's limits (stride 2 .. 8, 2 stride <= kernel <= 17)")


class DAPPMBranch(SgxBlock):
    """One branch's parameters and its two conv stages; DAPPM runs the branches (their pools are one launch over all of them)."""

    def __init__(self, kernel_size: int, stride: int, in_planes: int, branch_planes: int, inter_mode: str = "bilinear"):
        super().__init__()
        if inter_mode != "bilinear":
            raise NotImplementedError(f"DAPPMBranch on the HIP path: bilinear interpolation, got {inter_mode!r}")
        need_mult4("DAPPMBranch", "in_planes", in_planes)
        need_mult4("DAPPMBranch", "branch_planes", branch_planes)
        if stride > 1:
            _check_pool(kernel_size, stride)
        elif stride < 0:
            raise NotImplementedError(f"DAPPMBranch: stride {stride}")
        self.kernel_size, self.stride = kernel_size, stride
        self.down_scale = _BNReLUConv(0 if stride == 1 else 1, in_planes, branch_planes, 1)
        if stride != 1:
            self.process = _BNReLUConv(0, branch_planes, branch_planes, 3)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        raise NotImplementedError("DAPPMBranch holds a branch's parameters; on the HIP path the branches run inside DAPPM (their pools are one launch)")

    bwd = fwd


class DAPPM(SgxBlock):
    def __init__(self, in_planes: int, branch_planes: int, out_planes: int, kernel_sizes: list, strides: list, inter_mode: str = "bilinear"):
        super().__init__()
        assert len(kernel_sizes) == len(strides), "len of kernel_sizes and strides must be the same"
        need_mult4("DAPPM", "out_planes", out_planes)
        strides = [int(s) for s in strides]
        if not strides or strides[0] != 1 or any(s == 1 for s in strides[1:]) or strides.count(0) > 1:
            raise NotImplementedError(f"DAPPM on the HIP path: a stride-1 first branch, pooled branches behind it, at most one global; got strides {strides}")
        self.branches = Numbered([DAPPMBranch(int(k), s, in_planes, branch_planes, inter_mode) for k, s in zip(kernel_sizes, strides)])
        self._levels = [(int(k), s) for k, s in zip(kernel_sizes, strides) if s > 1]
        if len(self._levels) > 3:
            raise NotImplementedError(f"DAPPM on the HIP path: at most three window levels in one pyramid launch, got {len(self._levels)}")
        # which output of the pyramid launch each pooled branch reads: the window levels in order, the global level last
        self._pooled_of = [None] + [len(self._levels) if s == 0 else sum(1 for t in strides[1:i] if t > 1) for i, s in enumerate(strides) if i]
        self._glob = 0 in strides
        self.branch_planes = branch_planes
        self.compression = _BNReLUConv(0, branch_planes * len(strides), out_planes, 1)
        self.shortcut = _BNReLUConv(0, in_planes, out_planes, 1)

    def on_materialize(self):
        pass

    def fwd(self, x, out=None):
        if out is not None:  # (a convolution's addend shares its output's strides: the module returns a tensor of its own)
            raise NotImplementedError("DAPPM.fwd: out= is not supported")
        n, h, w, _ = x.shape
        tr, bp, branches = self.training, self.branch_planes, self.branches.blocks()
        pooled, parts = K.dappm_pool_fwd(x, self._levels, self._glob, want_stats=tr)
        cat = torch.empty(n, h, w, bp * len(branches), device=x.device, dtype=torch.float32)
        rec = StatsRecord(cat.shape[3], n * h * w, x.device, self.compression._parts()[0]._synced()) if tr else None

        def slice_out(i, res):  # a convolution that wrote slice i of the concat buffer: its epilogue's statistics go into the record
            if tr:
                rec.put(res[1], i * bp, n * h * w)
            return res[0] if tr else res

        prev = slice_out(0, branches[0].down_scale.run(x, parts[0] if tr else None, n * h * w, out=cat[..., :bp], stats=tr))
        sizes = []
        for i, br in enumerate(branches[1:], 1):
            j = self._pooled_of[i]
            p = pooled[j]
            u = br.down_scale.run(p, parts[1 + j] if tr else None, p.shape[0] * p.shape[1] * p.shape[2])
            s = K.resize_bilinear_fwd(u, (h, w), addend=prev, want_stats=tr)
            prev = slice_out(i, br.process.run(s[0] if tr else s, s[1] if tr else None, n * h * w, out=cat[..., i * bp:(i + 1) * bp], stats=tr))
            sizes.append(tuple(p.shape[1:3]))
        y = self.compression.run(cat, rec=rec)
        y = self.shortcut.run(x, parts[0] if tr else None, n * h * w, addend=y)
        self._ctx = (tuple(x.shape), sizes) if tr else None
        return y

    def bwd(self, dy, dx_out=None, accumulate=False, addend=None, need_dx=True):
        (x_shape, sizes), self._ctx = self._ctx, None
        if addend is not None:
            raise NotImplementedError("DAPPM.bwd: no addend")
        bp, branches = self.branch_planes, self.branches.blocks()
        a_short = self.shortcut.back(dy)
        dcat = self.compression.back(dy)
        d_pooled = [None] * (len(self._levels) + int(self._glob))
        carry = None  # the gradient the next branch's sum sends to this branch's output
        for i in range(len(branches) - 1, 0, -1):
            g = dcat[..., i * bp:(i + 1) * bp]
            ds = branches[i].process.back(g if carry is None else K.affine_act(g, r1=carry))
            du = K.resize_bilinear_bwd(ds, sizes[i - 1])
            d_pooled[self._pooled_of[i]] = branches[i].down_scale.back(du)
            carry = ds
        g = dcat[..., :bp]
        a_first = branches[0].down_scale.back(g if carry is None else K.affine_act(g, r1=carry))
        if not need_dx:
            return None
        nl = len(self._levels)
        return K.dappm_pool_bwd(d_pooled[:nl], self._levels, x_shape, d_global=d_pooled[nl] if self._glob else None, addends=[a_first, a_short], out=dx_out,
                                accumulate=accumulate)
