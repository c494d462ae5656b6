"""The squeeze-excitation kernels (csrc/se.hip: sgx_image_colsum, sgx_channel_gate, sgx_upsample2x_fwd / _bwd, sgx_bn_gate_act_fwd / _bwd_gate /
_bwd_data; csrc/half.hip: sgx_himage_colsum, sgx_hchannel_gate, sgx_hupsample2x_fwd) against plain torch in fp64 on the same fp32 (bf16-rounded)
operands, across their launch geometries: several pixel chunks, several channel strips with a part-filled last one, channel counts whose
float4 groups do not divide the workgroup, row blocks that straddle images, one-pixel images, channel-slice views of wider buffers, in-place
calls, and - on the chip only - problems larger than the capped grids, where the grid-stride loops make a second trip.  Both back ends run the
same shapes.  Every case first asserts, from the library's own size queries, the geometry it was chosen for.

Every comparison prints `SE_ERR <kernel> <quantity> <bar> <measured>` before it asserts (pytest -rP shows the lines).
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from test_half import _check as half_check  # the bf16 bars: an fp32-sum bound of 2e-5, one bf16 ulp, unchanged
from util import empty_nhwc, rel_err, to_nchw_cpu, to_nhwc

from super_gradients_amd import kernels as K

TOL = 2e-5       # element-wise results, of the tensor's max-abs (tests/test_kernels.py, tests/test_hswish_gate_dropout.py)
TOL_SUM = 1e-4   # per-image / per-channel sums: d pre and the column sums of the reduce rows (tests/test_hswish_gate_dropout.py)
TOL_DPRE = 5e-5  # image_colsum's gate-gradient form (tests/test_kernels.py::test_se_gate)
KINK = 1e-3      # no fp64 pre-activation of an input lies this close to a kink of the composition
CHUNK_ROWS = 512  # SE_CHUNK_ROWS, asserted through sgx_image_colsum_workspace
NAN = float("nan")


def hswish(t):
    return t * F.relu6(t + 3.0) / 6.0


GATES = {"hardsigmoid": lambda p: F.relu6(p + 3.0) / 6.0, "sigmoid": torch.sigmoid, "none": lambda p: p}
ACTS = {"relu": F.relu, "hswish": hswish, "none": lambda t: t}

# (N, H, W, C), pixel chunks per image, row blocks of the sweeps, and what the shape is there for
SHAPES = [
    # HW = 529: two pixel chunks, the second with 17 pixels; C4 = 18: RL = 14, 252 live lanes (MobileNetV3's 28x28x72 stage)
    SimpleNamespace(shape=(2, 23, 23, 72), chunks=2, nblk=17, straddle=True),
    # C4 = 66: two channel strips, the second with two live groups; M = 225: 4 row blocks of 57 rows, each straddling images of 45 pixels
    SimpleNamespace(shape=(5, 5, 9, 264), chunks=1, nblk=4, straddle=True),
    # one channel group, 256 row lanes, chunk boundary 512 | 1
    SimpleNamespace(shape=(1, 1, 513, 4), chunks=2, nblk=9, straddle=False),
    # HW = 512: exactly one full chunk
    SimpleNamespace(shape=(2, 16, 32, 8), chunks=1, nblk=16, straddle=False),
    # C4 = 257: five strips, the last with one live group; HW = 9 < RL
    SimpleNamespace(shape=(2, 3, 3, 1028), chunks=1, nblk=1, straddle=False),
    # HW = 1: the d = 1 form of the fast division; C4 = 38: RL = 6 (a RegNetY200 width)
    SimpleNamespace(shape=(4, 1, 1, 152), chunks=1, nblk=1, straddle=False),
    # strips of 64 + 30 groups (the RegNetY200 last stage); 7 row blocks of 56 rows against images of 196
    SimpleNamespace(shape=(2, 14, 14, 376), chunks=1, nblk=7, straddle=True),
]
SHAPE_IDS = ["x".join(map(str, s.shape)) for s in SHAPES]
BY_SHAPE = {s.shape: s for s in SHAPES}
LAYOUTS = ["slices", "contiguous"]
# (extra floats per pixel, channel offset) of operand k when it is a channel slice of a wider NaN-filled buffer: all multiples of 4 floats,
# a different pair per operand.  At least 256 floats follow every slice: a strip's worth of channel groups stored past C (a lost
# `c4 < C4` guard) then lands in the NaN surroundings of the same buffer, where the bit comparison reports it, even for the last pixel.
SLICE = [(264, 4), (272, 8), (260, 0), (280, 12), (268, 4), (276, 0), (284, 4), (296, 16)]


def _assert_geometry(case):
    """The geometry the case claims, from the library: a change of SE_CHUNK_ROWS or of the row-block rule fails here."""
    n, h, w, c = case.shape
    hw, m = h * w, n * h * w
    assert case.chunks == -(-hw // CHUNK_ROWS)
    assert K.lib().sgx_image_colsum_workspace(n, hw, c) == n * case.chunks * c * 4 + 256
    assert K.lib().sgx_bn_gate_act_bwd_gate_workspace(n, hw, c) == n * case.chunks * c * 4 + 256
    assert K.stats_blocks(m) == case.nblk
    rows_per_blk = -(-m // case.nblk)
    assert (case.nblk > 1 and n > 1 and rows_per_blk % hw != 0 and hw % rows_per_blk != 0) == case.straddle


# --------------------------------------------------------------------------------------------- operands and comparisons
def _operand(t_nchw, dev, layout, k):
    c = t_nchw.shape[1]
    if layout == "contiguous":
        return to_nhwc(t_nchw.clone(), dev)  # (a one-pixel map is already contiguous as NHWC: never hand out the shared case's own memory)
    pad, off = SLICE[k]
    return to_nhwc(t_nchw, dev, ld_pix=c + pad, c_off=off)


def _result(shape, dev, layout, k):
    """An NaN-filled output view: whatever a kernel does not write stays NaN, whatever it writes outside the view shows in the base."""
    n, h, w, c = shape
    if layout == "contiguous":
        return empty_nhwc(n, h, w, c, dev).fill_(NAN)
    pad, off = SLICE[k]
    return empty_nhwc(n, h, w, c, dev, ld_pix=c + pad, c_off=off)


def _base(v):
    return v if v._base is None else v._base


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _surround(v):
    """The bits of v's whole base buffer with v's own channels blanked: equal before and after a call that may only write v."""
    base = _base(v)
    b = base.clone()
    lo = (v.storage_offset() - base.storage_offset()) % base.shape[-1]
    b[..., lo:lo + v.shape[-1]] = 0
    return _bits(b).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _close(got, ref, tol, kernel, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"{kernel} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    e = rel_err(got, ref)
    print(f"SE_ERR {kernel} {what} {tol:g} {e:.3e}")
    assert e <= tol, f"{kernel} {what}: max err {e:.3e} of the tensor's max-abs > {tol}"


def _draw_pre(g, n, c, gate=None):
    """Gate pre-activations [n, c] on both sides of -3 and 3, none within KINK of +-3 (the hard-sigmoid's kinks).  With `gate` (the fused
    sweeps) also no gate value in (0, 0.02): s * z could not be kept away from the activation's kink at 0 otherwise."""
    pre = torch.randn(n, c, generator=g) * 2.5
    pre.view(-1)[:3] = torch.tensor([-3.7, 3.6, 0.8])
    for _ in range(50):
        p = pre.double()
        bad = (p.abs() - 3.0).abs() < KINK
        if gate is not None:
            s = GATES[gate](p).abs()
            bad |= (s > 0) & (s < 0.02)
        if not bool(bad.any()):
            break
        pre = torch.where(bad, torch.randn(n, c, generator=g) * 2.5, pre)
    p = pre.double()
    assert not bool(((p.abs() - 3.0).abs() < KINK).any())
    assert bool((p < -3).any()) and bool((p > 3).any()) and bool(((p > -3) & (p < 3)).any())
    return pre


def _near_act_kink(t, act):
    if act == "relu":
        return t.abs() < KINK
    if act == "hswish":
        return ((t - 3.0).abs() < KINK) | ((t + 3.0).abs() < KINK)
    return torch.zeros_like(t, dtype=torch.bool)


def _seed(*parts):
    return sum((i + 1) * 7919 * (sum(map(ord, p)) if isinstance(p, str) else int(p)) for i, p in enumerate(parts)) % (2 ** 31)


# --------------------------------------------------------------------------------------------- the fused sweeps
@functools.lru_cache(maxsize=None)
def _sweep_case(shape, gate, act, affine):
    """Inputs and the fp64 autograd reference of y = act(f(pre) * (scale * x + shift)), built once per case and shared by both back ends
    and both layouts (nothing here is written afterwards).  Input condition, checked in fp64 on the CPU: no s * z within KINK of a kink of
    the activation (0 for relu, +-3 for hard-swish) and no gate pre-activation within KINK of +-3, so that the derivative is well defined.
    The one exemption: elements whose hard-sigmoid gate is saturated at exactly 0 have s * z = 0, and there y is identically 0 in a
    neighbourhood of the inputs (pre is at least KINK below -3): dz = s * act' = 0 and d pre = f' * ... = 0 whatever act'(0) is taken to be.
    No output element is excluded from any comparison."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(_seed(n, h, w, c, gate, act, int(affine)))
    pre = _draw_pre(g, n, c, gate)
    scale = torch.rand(c, generator=g) + 0.5 if affine else None
    shift = torch.randn(c, generator=g) if affine else None
    s = GATES[gate](pre.double()).view(n, c, 1, 1)

    def sz(x):
        z = x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) if affine else x.double()
        return s * z

    x = torch.randn(n, c, h, w, generator=g) * 3.0
    for _ in range(50):
        bad = _near_act_kink(sz(x), act) & (s != 0)
        if not bool(bad.any()):
            break
        x = torch.where(bad, torch.randn(n, c, h, w, generator=g) * 3.0, x)
    t = sz(x)
    assert not bool((_near_act_kink(t, act) & (s != 0)).any())
    if act == "relu":
        assert bool((t < 0).any()) and bool((t > 0).any())
    if act == "hswish":
        assert bool((t < -3).any()) and bool((t > 3).any()) and bool(((t > -3) & (t < 3)).any())
    dy, dmean, mean = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, generator=g), torch.randn(c, generator=g)
    xd, pd = x.double(), pre.double().requires_grad_(True)
    z = xd * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) if affine else xd.clone()
    z.requires_grad_(True)
    y = ACTS[act](GATES[gate](pd).view(n, c, 1, 1) * z)
    gz, gp = torch.autograd.grad(y, (z, pd), dy.double())
    return SimpleNamespace(x=x, pre=pre, scale=scale, shift=shift, dy=dy, dmean=dmean, mean=mean, y=y.detach(), gz=gz, gp=gp,
                           gz_mean=gz + dmean.double().view(n, c, 1, 1) / (h * w))


FULL = [SHAPES[0].shape, SHAPES[1].shape]  # the full gate x activation x affine product on these two ...
SWEEP_CASES = [(s, g, a, f) for s in FULL for g in GATES for a in ACTS for f in (True, False)] + [
    # ... and one combination on the rest: every gate and every activation at least twice
    ((1, 1, 513, 4), "sigmoid", "hswish", True),
    ((2, 16, 32, 8), "hardsigmoid", "relu", False),
    ((2, 3, 3, 1028), "none", "hswish", True),
    ((4, 1, 1, 152), "hardsigmoid", "none", True),
    ((4, 1, 1, 152), "none", "none", False),
    ((2, 14, 14, 376), "sigmoid", "relu", False),
]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,gate,act,affine", SWEEP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_sweeps(backend, shape, gate, act, affine, layout):
    """sgx_bn_gate_act_fwd / _bwd_gate / _bwd_data against fp64 autograd; the reduce rows against sgx_bn_bwd_reduce (bits) and fp64 sums;
    repeatability; the in-place form; nothing written outside a channel slice."""
    _assert_geometry(BY_SHAPE[shape])
    n, h, w, c = shape
    hw, m = h * w, n * h * w
    cs = _sweep_case(shape, gate, act, affine)
    dev = lambda t: None if t is None else t.to(backend)  # noqa: E731
    pre, scale, shift, dmean, mean = dev(cs.pre), dev(cs.scale), dev(cs.shift), dev(cs.dmean), dev(cs.mean)
    xk, dyk = _operand(cs.x, backend, layout, 0), _operand(cs.dy, backend, layout, 1)
    tag = f"{gate}/{act}/{'affine' if affine else 'folded'}"

    out = _result(shape, backend, layout, 2)
    before = _surround(out)
    assert K.bn_gate_act_fwd(xk, scale, shift, pre, gate, act=act, out=out) is out
    assert torch.equal(_surround(out), before), "bn_gate_act_fwd wrote outside its channel slice"
    _close(to_nchw_cpu(out), cs.y, TOL, "bn_gate_act_fwd", f"y[{tag}]")
    again = _result(shape, backend, layout, 3)
    K.bn_gate_act_fwd(xk, scale, shift, pre, gate, act=act, out=again)
    assert _same_bits(out, again), "bn_gate_act_fwd: a second call gives other bits"

    dpre = K.bn_gate_act_bwd_gate(dyk, xk, scale, shift, pre, gate, act=act)
    _close(dpre, cs.gp, TOL_SUM, "bn_gate_act_bwd_gate", f"dpre[{tag}]")
    assert _same_bits(dpre, K.bn_gate_act_bwd_gate(dyk, xk, scale, shift, pre, gate, act=act)), "bn_gate_act_bwd_gate: a second call gives other bits"

    dz = _result(shape, backend, layout, 4)
    before = _surround(dz)
    _, parts = K.bn_gate_act_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=dz, want_parts=True)
    assert torch.equal(_surround(dz), before), "bn_gate_act_bwd_data wrote outside its channel slice"
    _close(to_nchw_cpu(dz), cs.gz_mean, TOL, "bn_gate_act_bwd_data", f"dz+dmean/HW[{tag}]")
    plain = _result(shape, backend, layout, 5)
    K.bn_gate_act_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, out=plain)
    _close(to_nchw_cpu(plain), cs.gz, TOL, "bn_gate_act_bwd_data", f"dz[{tag}]")

    assert tuple(parts.shape) == (2, K.stats_blocks(m), c)
    rows = torch.full((2, K.stats_blocks(m), c), NAN, device=backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    K.check(K.lib().sgx_bn_bwd_reduce(K.ptr(dz), K.rows(dz)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(one), K.ptr(zero), K.ptr(mean), m, c, 0, K.ptr(rows),
                                      K.stream()), "sgx_bn_bwd_reduce")
    assert _same_bits(parts, rows), "reduce rows differ from bn_bwd_reduce's"
    dzd = to_nchw_cpu(dz).double()
    _close(parts[0].sum(0), dzd.sum((0, 2, 3)), TOL_SUM, "bn_gate_act_bwd_data", f"rows:sum-dz[{tag}]")
    _close(parts[1].sum(0), (dzd * (cs.x.double() - cs.mean.double().view(1, -1, 1, 1))).sum((0, 2, 3)), TOL_SUM, "bn_gate_act_bwd_data", f"rows:sum-dz(x-mean)[{tag}]")

    dz2 = _result(shape, backend, layout, 6)
    _, parts2 = K.bn_gate_act_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=dz2, want_parts=True)
    assert _same_bits(dz, dz2) and _same_bits(parts, parts2), "bn_gate_act_bwd_data: a second call gives other bits"
    inplace = _operand(cs.dy, backend, layout, 7)
    before = _surround(inplace)
    r, parts3 = K.bn_gate_act_bwd_data(inplace, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=inplace, want_parts=True)
    assert r is inplace and _same_bits(inplace, dz) and _same_bits(parts3, parts), "bn_gate_act_bwd_data(out=dy) differs from the out-of-place call"
    assert torch.equal(_surround(inplace), before), "bn_gate_act_bwd_data(out=dy) wrote outside its channel slice"


# --------------------------------------------------------------------------------------------- image_colsum
@functools.lru_cache(maxsize=None)
def _colsum_case(shape):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(_seed(n, h, w, c, "colsum"))
    u, v, pre = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g), _draw_pre(g, n, c)
    s = (u.double() * v.double()).sum((2, 3))
    grad = {}
    for gate, f in GATES.items():
        p = pre.double().requires_grad_(True)
        (grad[gate],) = torch.autograd.grad(f(p), p, s)  # f'(pre) * sum u * v
    return SimpleNamespace(u=u, v=v, pre=pre, mean=u.double().mean((2, 3)), grad=grad)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_image_colsum(backend, case, layout):
    """The plain per-image mean and the SE gate gradient f'(pre) * sum u * v, u and v with different strides."""
    _assert_geometry(case)
    n, h, w, c = case.shape
    cs = _colsum_case(case.shape)
    u, v, pre = _operand(cs.u, backend, layout, 0), _operand(cs.v, backend, layout, 3), cs.pre.to(backend)
    if layout == "slices":
        assert K.nhwc_strides(u) != K.nhwc_strides(v)
    mean = K.image_colsum(u, scale=1.0 / (h * w))
    _close(mean, cs.mean, TOL, "image_colsum", "mean")
    assert _same_bits(mean, K.image_colsum(u, scale=1.0 / (h * w))), "image_colsum: a second call gives other bits"
    for gate in GATES:
        _close(K.image_colsum(u, v=v, pre=pre, gate=gate), cs.grad[gate], TOL_DPRE, "image_colsum", f"dpre[{gate}]")


# --------------------------------------------------------------------------------------------- channel_gate
@functools.lru_cache(maxsize=None)
def _gate_case(shape):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(_seed(n, h, w, c, "gate"))
    x, pre = torch.randn(n, c, h, w, generator=g), _draw_pre(g, n, c)
    bias, base = torch.randn(n, c, generator=g), torch.randn(n, c, h, w, generator=g)
    y = {gate: x.double() * f(pre.double()).view(n, c, 1, 1) for gate, f in GATES.items()}
    return SimpleNamespace(x=x, pre=pre, bias=bias, base=base, y=y)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_channel_gate(backend, case, layout):
    """y (+)= x * f(pre) + bias_scale * bias: plain (every gate), with the bias, accumulated onto a base, and in place."""
    n, h, w, c = case.shape
    cs = _gate_case(case.shape)
    x, pre, bias = _operand(cs.x, backend, layout, 0), cs.pre.to(backend), cs.bias.to(backend)
    for gate in GATES:
        out = _result(case.shape, backend, layout, 1)
        before = _surround(out)
        assert K.channel_gate(x, pre, gate, out=out) is out
        assert torch.equal(_surround(out), before), "channel_gate wrote outside its channel slice"
        _close(to_nchw_cpu(out), cs.y[gate], TOL, "channel_gate", f"plain[{gate}]")
    gate = list(GATES)[SHAPES.index(case) % 3]
    bterm = 0.25 * cs.bias.double().view(n, c, 1, 1)
    out = _result(case.shape, backend, layout, 2)
    K.channel_gate(x, pre, gate, bias=bias, bias_scale=0.25, out=out)
    _close(to_nchw_cpu(out), cs.y[gate] + bterm, TOL, "channel_gate", f"bias[{gate}]")
    acc = _operand(cs.base, backend, layout, 4)
    before = _surround(acc)
    K.channel_gate(x, pre, gate, bias=bias, bias_scale=0.25, out=acc, accumulate=True)
    assert torch.equal(_surround(acc), before), "channel_gate(accumulate) wrote outside its channel slice"
    _close(to_nchw_cpu(acc), cs.base.double() + cs.y[gate] + bterm, TOL, "channel_gate", f"accumulate+bias[{gate}]")
    inplace = _operand(cs.x, backend, layout, 5)
    before = _surround(inplace)
    K.channel_gate(inplace, pre, gate, out=inplace)
    assert torch.equal(_surround(inplace), before), "channel_gate in place wrote outside its channel slice"
    _close(to_nchw_cpu(inplace), cs.y[gate], TOL, "channel_gate", f"in-place[{gate}]")


# --------------------------------------------------------------------------------------------- nearest x2 up-sampling
UP_SHAPES = [s.shape for s in SHAPES] + [(2, 1, 1, 4), (1, 3, 5, 260)]  # (H, W: the INPUT map) + one group per pixel; a second strip of one group


@functools.lru_cache(maxsize=None)
def _up_case(shape):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(_seed(n, h, w, c, "up"))
    x, dy, base = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, 2 * h, 2 * w, generator=g), torch.randn(n, c, h, w, generator=g)
    gx = dy.double().view(n, c, h, 2, w, 2).sum((3, 5))
    return SimpleNamespace(x=x, dy=dy, base=base, up=x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), gx=gx)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample2x(backend, shape, layout):
    """Forward: a copy, bit-exact against repeat_interleave.  Backward: the sum of the four, also accumulated onto a base."""
    n, h, w, c = shape
    cs = _up_case(shape)
    up = _result((n, 2 * h, 2 * w, c), backend, layout, 1)
    before = _surround(up)
    assert K.upsample2x_fwd(_operand(cs.x, backend, layout, 0), out=up) is up
    assert torch.equal(_surround(up), before), "upsample2x_fwd wrote outside its channel slice"
    assert _same_bits(to_nchw_cpu(up), cs.up), "nearest up-sampling is a copy: bit-exact"
    dy = _operand(cs.dy, backend, layout, 2)
    dx = _result(shape, backend, layout, 3)
    before = _surround(dx)
    K.upsample2x_bwd(dy, out=dx)
    assert torch.equal(_surround(dx), before), "upsample2x_bwd wrote outside its channel slice"
    _close(to_nchw_cpu(dx), cs.gx, 1e-6, "upsample2x_bwd", "dx")
    acc = _operand(cs.base, backend, layout, 4)
    before = _surround(acc)
    K.upsample2x_bwd(dy, out=acc, accumulate=True)
    assert torch.equal(_surround(acc), before), "upsample2x_bwd(accumulate) wrote outside its channel slice"
    _close(to_nchw_cpu(acc), cs.base.double() + cs.gx, 1e-6, "upsample2x_bwd", "accumulate")


# --------------------------------------------------------------------------------------------- the bf16 trio
BF = torch.bfloat16


def _bf_slice(src_nhwc, dev, pad, off):
    """src (bf16 NHWC; None: nothing copied) as channels off.. of an NaN-filled buffer that is `pad` channels wider (multiples of 8)."""
    n, h, w, c = src_nhwc if isinstance(src_nhwc, tuple) else src_nhwc.shape
    v = torch.full((n, h, w, c + pad), NAN, dtype=BF, device=dev)[..., off:off + c]
    if not isinstance(src_nhwc, tuple):
        v.copy_(src_nhwc.to(dev))
    return v


@functools.lru_cache(maxsize=None)
def _half_case(c, h, w):
    g = torch.Generator().manual_seed(_seed(c, h, w, "half"))
    x = torch.randn(2, h, w, c, generator=g).to(BF)
    pre = _draw_pre(g, 2, c)
    xr = x.double()
    return SimpleNamespace(x=x, pre=pre, mean=xr.mean((1, 2)), y={gate: xr * f(pre.double()).view(2, 1, 1, c) for gate, f in GATES.items()},
                           up=x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))


# C = 8: one octet; 64: one full workgroup of channels; 72: a second 64-channel workgroup with one live octet; 200: a part-filled last one.
# 1x1, 1x31 (fewer pixels than the 32 pixel lanes), 3x11 (HW = 33: a second trip for one pixel lane only), 23x23
@pytest.mark.parametrize("hw", [(1, 1), (1, 31), (3, 11), (23, 23)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("c", [8, 64, 72, 200])
def test_half_trio(backend, c, hw):
    """sgx_himage_colsum, sgx_hchannel_gate, sgx_hupsample2x_fwd on channel slices of wider bf16 buffers, against fp64 on the bf16-rounded
    operands with tests/test_half.py's bars.  (hcolsum_kernel's guard `c < C` only keeps the lanes of a part-filled workgroup from reading
    past C: their sums are never folded into an output, so no comparison of values can see that guard.)"""
    h, w = hw
    cs = _half_case(c, h, w)
    x, pre = _bf_slice(cs.x, backend, 16, 8), cs.pre.to(backend)
    mean = K.image_colsum(x, scale=1.0 / (h * w))
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (2, c) and bool(torch.isfinite(mean).all())
    print(f"SE_ERR himage_colsum mean 2e-05 {rel_err(mean, cs.mean):.3e}")
    half_check(mean.cpu(), cs.mean, "himage_colsum")
    for gate in GATES:
        out = _bf_slice((2, h, w, c), backend, 24, 16)
        before = _surround(out)
        assert K.channel_gate(x, pre, gate, out=out) is out
        assert torch.equal(_surround(out), before), "hchannel_gate wrote outside its channel slice"
        assert bool(torch.isfinite(out.float()).all())
        half_check(out.cpu(), cs.y[gate], f"hchannel_gate[{gate}]")
    up = _bf_slice((2, 2 * h, 2 * w, c), backend, 8, 0)
    before = _surround(up)
    K.upsample2x_fwd(x, out=up)
    assert torch.equal(_surround(up), before), "hupsample2x_fwd wrote outside its channel slice"
    assert _same_bits(up.cpu(), cs.up), "nearest up-sampling is a copy: bit-exact"


# --------------------------------------------------------------------------------------------- grid wrap (chip only)
# The grids of channel_gate, upsample2x_fwd / _bwd, hchannel_gate and hupsample2x are capped at 16384 workgroups of 256 threads; past
# 16384 * 256 float4 (bf16: 8-channel) groups a thread makes a second trip of its grid-stride loop.  These are the smallest problems past the
# cap in which only part of the grid makes it.  The host emulation runs one fiber per thread and cannot run 4 M of them in seconds; these
# cases are the only cover of those loops.  References: torch's own ops on the device; outputs are pre-filled with NaN.
GRID_CAP = 16384 * 256


def _randn(shape, dev, seed, dtype=torch.float32):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).to(dtype)


@pytest.mark.gpu
def test_grid_wrap_channel_gate(gpu_device):
    n, h, w, c = 1, 1025, 1024, 16
    assert GRID_CAP < n * h * w * (c // 4) < 2 * GRID_CAP
    x, pre = _randn((n, h, w, c), gpu_device, 1), _randn((n, c), gpu_device, 2) * 2.5
    out = torch.full_like(x, NAN)
    K.channel_gate(x, pre, "sigmoid", out=out)
    ref = x * torch.sigmoid(pre).view(n, 1, 1, c)
    assert bool(torch.isfinite(out).all()), "channel_gate left elements unwritten past the grid cap"
    e = float((out - ref).abs().max() / ref.abs().max())
    print(f"SE_ERR channel_gate grid-wrap {TOL:g} {e:.3e}")
    assert e <= TOL


@pytest.mark.gpu
def test_grid_wrap_upsample2x_fwd(gpu_device):
    n, h, w, c = 1, 513, 512, 64
    assert GRID_CAP < n * h * w * (c // 4) < 2 * GRID_CAP
    x = _randn((n, h, w, c), gpu_device, 3)
    out = torch.full((n, 2 * h, 2 * w, c), NAN, device=gpu_device)
    K.upsample2x_fwd(x, out=out)
    assert torch.equal(out, x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))


@pytest.mark.gpu
def test_grid_wrap_upsample2x_bwd(gpu_device):
    n, h, w, c = 1, 513, 512, 64
    assert GRID_CAP < n * h * w * (c // 4) < 2 * GRID_CAP
    dy = _randn((n, 2 * h, 2 * w, c), gpu_device, 4)
    dx = torch.full((n, h, w, c), NAN, device=gpu_device)
    K.upsample2x_bwd(dy, out=dx)
    ref = (dy[:, 0::2, 0::2] + dy[:, 0::2, 1::2]) + (dy[:, 1::2, 0::2] + dy[:, 1::2, 1::2])  # the kernel's own order: the same fp32 roundings
    assert torch.equal(dx, ref)


@pytest.mark.gpu
def test_grid_wrap_hchannel_gate(gpu_device):
    n, h, w, c = 1, 1025, 1024, 32
    assert GRID_CAP < n * h * w * (c // 8) < 2 * GRID_CAP
    x, pre = _randn((n, h, w, c), gpu_device, 5, BF), _randn((n, c), gpu_device, 6) * 2.5
    out = torch.full_like(x, NAN)
    K.channel_gate(x, pre, "none", out=out)
    # gate none: one fp32 product rounded once to bf16, nearest-even on both sides
    assert torch.equal(out, (x.float() * pre.view(n, 1, 1, c)).to(BF))


@pytest.mark.gpu
def test_grid_wrap_hupsample2x_fwd(gpu_device):
    n, h, w, c = 1, 513, 512, 32  # (this kernel counts OUTPUT pixels: a quarter of the gate's input)
    assert GRID_CAP < n * 4 * h * w * (c // 8) < 2 * GRID_CAP
    x = _randn((n, h, w, c), gpu_device, 7, BF)
    out = torch.full((n, 2 * h, 2 * w, c), NAN, dtype=BF, device=gpu_device)
    K.upsample2x_fwd(x, out=out)
    assert torch.equal(out, x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))


# --------------------------------------------------------------------------------------------- rejections
# Float offsets of the operands inside one zero-filled buffer (N = 2, H = W = 2, C = 8: tensors of 64 floats, the up-sampled one 256), all
# 16-byte aligned and far from the buffer's end: were a check missing, the launch it lets through would still stay inside the buffer.
_AT = dict(a=0, b=512, o=1024, pre=1536, bias=1600, dmean=1664, scale=1728, shift=1792, mean=1856, vec=1920, parts=2048, ws=4096)
_LDS = dict(a_lp=8, a_li=32, b_lp=8, b_li=32, o_lp=8, o_li=32, up_li=128)


def _rejections(L, base, what, call, pointers, strides):
    """`call(**args)` with each pointer off by 4 and by 8 bytes and each stride off by 2 floats, one defect at a time: -1 and a message."""
    good = {k: base + 4 * v for k, v in _AT.items()}
    good.update(_LDS)
    tried = 0
    for name, deltas in [(p, (4, 8)) for p in pointers] + [(s, (2,)) for s in strides]:
        for d in deltas:
            args = dict(good)
            args[name] += d
            rc = call(**args)
            msg = (L.sgx_last_error() or b"").decode()
            assert rc == -1 and what in msg and "16 bytes" in msg, f"{what}: {name} off by {d}: status {rc}, message {msg!r}"
            tried += 1
    return tried


def test_rejects_unaligned_addresses_and_strides(backend):
    """Every fp32 entry point of se.hip moves float4: an address that is not a multiple of 16 bytes (tensors, the [N][C] / [C] vectors, the
    workspace) or a stride that is not a multiple of 4 floats is SGX_ERR_BAD_ARG with a message, and nothing is launched - the buffer
    keeps its bits."""
    L, st = K.lib(), K.stream()
    buf = torch.zeros(8192, device=backend)
    base = K.ptr(buf)
    assert base % 16 == 0
    N, H, W, C, HW, wsb = 2, 2, 2, 8, 4, 4096 * 4
    tried = _rejections(L, base, "image_colsum", lambda **a: L.sgx_image_colsum(N, HW, C, a["a"], a["a_lp"], a["a_li"], a["b"], a["b_lp"], a["b_li"], 1.0, a["pre"], 1,
                                                                                 a["vec"], a["ws"], wsb, st),
                        ["a", "b", "pre", "vec", "ws"], ["a_lp", "a_li", "b_lp", "b_li"])
    tried += _rejections(L, base, "channel_gate", lambda **a: L.sgx_channel_gate(N, HW, C, a["a"], a["a_lp"], a["a_li"], a["pre"], 1, a["bias"], 0.5, a["o"], a["o_lp"],
                                                                                  a["o_li"], 0, st),
                         ["a", "o", "pre", "bias"], ["a_lp", "a_li", "o_lp", "o_li"])
    tried += _rejections(L, base, "upsample2x_fwd", lambda **a: L.sgx_upsample2x_fwd(N, H, W, C, a["a"], a["a_lp"], a["a_li"], a["o"], a["o_lp"], a["up_li"], st),
                         ["a", "o"], ["a_lp", "a_li", "o_lp", "up_li"])
    tried += _rejections(L, base, "upsample2x_bwd", lambda **a: L.sgx_upsample2x_bwd(N, H, W, C, a["o"], a["o_lp"], a["up_li"], a["a"], a["a_lp"], a["a_li"], 0, st),
                         ["a", "o"], ["a_lp", "a_li", "o_lp", "up_li"])
    tried += _rejections(L, base, "bn_gate_act_fwd", lambda **a: L.sgx_bn_gate_act_fwd(a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 1, a["o"], a["o_lp"], N, HW, C, 4, st),
                         ["a", "o", "scale", "shift", "pre"], ["a_lp", "o_lp"])
    tried += _rejections(L, base, "bn_gate_act_bwd_gate", lambda **a: L.sgx_bn_gate_act_bwd_gate(a["b"], a["b_lp"], a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 1, 4,
                                                                                                  a["vec"], N, HW, C, a["ws"], wsb, st),
                         ["a", "b", "scale", "shift", "pre", "vec", "ws"], ["a_lp", "b_lp"])
    tried += _rejections(L, base, "bn_gate_act_bwd_data", lambda **a: L.sgx_bn_gate_act_bwd_data(a["b"], a["b_lp"], a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 1, 4,
                                                                                                  a["dmean"], a["o"], a["o_lp"], a["mean"], a["parts"], N, HW, C, st),
                         ["a", "b", "o", "scale", "shift", "pre", "dmean", "mean", "parts"], ["a_lp", "b_lp", "o_lp"])
    assert tried == 14 + 12 + 8 + 8 + 12 + 16 + 21
    assert bool((buf.view(torch.int32) == 0).all()), "a rejected call wrote to its buffers"
