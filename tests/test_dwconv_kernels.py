"""The depthwise 3x3 kernels (csrc/pool.hip: sgx_dwconv3x3_fwd / _bwd_data / _bwd_weight) and ReLU6 in the sweeps, against plain torch in fp64
(F.conv2d(groups=C) and autograd), on the chip and on the host emulation of the same sources."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5  # (tests/test_kernels.py's bar for element-wise sweeps; the sums here have nine terms)
TOL_WGRAD = 1e-4  # (the bar tests/test_kernels.py holds conv2d_bwd_weight to)
ACTS = {"relu": F.relu, "relu6": F.relu6, "silu": F.silu, None: lambda t: t}
# (N, H, W, C): odd and even extents under stride 2, maps where every pixel is an edge, several row blocks and channel-group rounds, the widest layer
GPU_SHAPES = [(3, 23, 19, 96), (2, 8, 8, 32), (2, 7, 7, 960), (1, 2, 2, 1296), (2, 1, 1, 16)]
EMU_SHAPES = [(2, 5, 3, 16), (1, 2, 2, 48), (2, 1, 1, 16)]
N_SHAPES = max(len(GPU_SHAPES), len(EMU_SHAPES))


def _shape(backend, i):
    """(the emulation has fewer shapes than the chip: the last indices run its first shapes again)"""
    shapes = GPU_SHAPES if backend.type == "cuda" else EMU_SHAPES
    return shapes[i % len(shapes)]


_CASES = {}


def _case(shape, stride):
    """Seeded operands and the fp64 reference of one problem (computed once, shared by the tests, never modified)."""
    key = (shape, stride)
    if key not in _CASES:
        n, h, w, c = shape
        g = torch.Generator().manual_seed(17 + 31 * stride + c + 7 * h)
        x = torch.randn(n, c, h, w, generator=g)
        wt = torch.randn(c, 1, 3, 3, generator=g) / 3.0
        bias = torch.randn(c, generator=g) * 0.5
        xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
        y = F.conv2d(xd, wd, None, stride, 1, groups=c)
        dy = torch.randn(y.shape, generator=g)
        dx, dw = torch.autograd.grad(y, (xd, wd), dy.double())
        _CASES[key] = dict(x=x, w=wt, bias=bias, y=y.detach(), dy=dy, dx=dx, dw=dw)
    return _CASES[key]


def _strided(strided, c):
    return dict(ld_pix=c + 8, c_off=4) if strided else {}


def _finalized(parts, M, backend):
    """mean / biased variance out of bn_finalize - the consumer of the rows in the blocks (tests/test_repvgg_kernels.py's scheme)."""
    c = parts.shape[2]
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    eps = 1e-5
    _, _, mean, invstd = K.bn_finalize(parts, M, one, zero, eps, 0.1, zero.clone(), one.clone())
    return mean.cpu().double(), 1.0 / invstd.cpu().double() ** 2 - eps


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_forward(backend, i, stride, strided):
    shape = _shape(backend, i)
    n, h, w, c = shape
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    wk = K.to_dw(fx["w"].to(backend))
    ho, wo = fx["y"].shape[2:]
    out = empty_nhwc(n, ho, wo, c, backend, **_strided(strided, c))
    y = K.dwconv3x3_fwd(x, wk, out=out, stride=stride)
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), fx["y"].float(), TOL, "dwconv forward")


@pytest.mark.parametrize("act", ["relu", "relu6", "silu", None])
@pytest.mark.parametrize("stride", [1, 2])
def test_forward_bias_act_epilogue(backend, stride, act):
    shape = _shape(backend, 0)
    fx = _case(shape, stride)
    ref = ACTS[act](fx["y"] * 4.0 + fx["bias"].double().view(1, -1, 1, 1))  # (x 4: pre-activations on both sides of 6)
    y = K.dwconv3x3_fwd(to_nhwc(fx["x"], backend), K.to_dw((fx["w"] * 4.0).to(backend)), bias=fx["bias"].to(backend), act=act, stride=stride)
    assert_close(to_nchw_cpu(y), ref.float(), TOL, f"act(dwconv + bias), {act}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_statistics_rows(backend, i, stride, strided):
    """[2][sgx_dwconv3x3_stat_blocks][C] rows of the stored y: what bn_finalize makes of them, their column sums, and the same bits on a second call."""
    shape = _shape(backend, i)
    n, h, w, c = shape
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    wk = K.to_dw(fx["w"].to(backend))
    y, parts = K.dwconv3x3_fwd(x, wk, stride=stride, stat_partials=True)
    d = K.conv_desc(x, c, 3, 3, stride, 1, y)
    assert tuple(parts.shape) == (2, K.lib().sgx_dwconv3x3_stat_blocks(d.ref), c)
    assert torch.equal(y.cpu(), K.dwconv3x3_fwd(x, wk, stride=stride).cpu()), "the statistics output changes what is stored"
    stored = to_nchw_cpu(y).double()
    M = stored.shape[0] * stored.shape[2] * stored.shape[3]
    assert_close(parts[0].sum(0).cpu(), stored.sum((0, 2, 3)).float(), 1e-4, "sum y")
    assert_close(parts[1].sum(0).cpu(), (stored * stored).sum((0, 2, 3)).float(), 1e-4, "sum y^2")
    if M > 1:
        mean, var = _finalized(parts, M, backend)
        assert_close(mean, stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
        assert_close(var, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
    _, again = K.dwconv3x3_fwd(x, wk, stride=stride, stat_partials=True)
    assert torch.equal(parts.cpu(), again.cpu()), "statistics rows differ between two calls"


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_data_gradient(backend, i, stride, strided):
    shape = _shape(backend, i)
    n, h, w, c = shape
    fx = _case(shape, stride)
    dy = to_nhwc(fx["dy"], backend, **_strided(strided, c))
    wk = K.to_dw(fx["w"].to(backend))
    out = empty_nhwc(n, h, w, c, backend, **_strided(strided, c))
    dx = K.dwconv3x3_bwd_data(dy, wk, (n, h, w, c), stride=stride, out=out)
    assert dx.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(dx), fx["dx"].float(), TOL, "dwconv data gradient")
    base = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(3))
    acc = to_nhwc(base.clone(), backend, **_strided(strided, c))  # (a clone: on a 1 x 1 map the NHWC view of a CPU tensor is the tensor itself)
    K.dwconv3x3_bwd_data(dy, wk, (n, h, w, c), stride=stride, out=acc, accumulate=True)
    assert_close(to_nchw_cpu(acc), (fx["dx"] + base.double()).float(), TOL, "dwconv data gradient, accumulate")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_weight_gradient(backend, i, stride, strided):
    """Against fp64; twice on a zeroed dw gives twice the gradient (it accumulates); two calls on the same inputs give the same bits."""
    shape = _shape(backend, i)
    n, h, w, c = shape
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    dy = to_nhwc(fx["dy"], backend, **_strided(strided, c))
    dw = K.dw_empty(c, backend)
    dw.zero_()
    K.dwconv3x3_bwd_weight(x, dy, dw, stride=stride)
    once = dw.cpu().clone()
    assert_close(once, fx["dw"].float(), TOL_WGRAD, "dwconv weight gradient")
    K.dwconv3x3_bwd_weight(x, dy, dw, stride=stride)
    assert_close(dw.cpu(), 2.0 * fx["dw"].float(), TOL_WGRAD, "dwconv weight gradient, second call accumulates")
    dw2 = K.dw_empty(c, backend)
    dw2.zero_()
    K.dwconv3x3_bwd_weight(x, dy, dw2, stride=stride)
    assert torch.equal(dw2.cpu(), once), "weight gradient differs between two calls"


# The strip height TH (rows a thread walks with its window in registers) is 8, halved down to 2 until a launch has 262 144 threads (65 536 for
# the weight gradient): the shapes above all run TH = 2 - one or two rows per strip.  These run what batch 64 at 224 x 224 runs: TH = 8 and
# TH = 4, several rows carried through the window, partial last strips (127 = 15 x 8 + 7, 63 = 15 x 4 + 3).  (kernel, stride, shape, TH)
TALL = [("fwd", 1, (1, 127, 128, 512), 8), ("fwd", 2, (1, 255, 256, 512), 8), ("fwd", 1, (1, 63, 128, 512), 4),
        ("dgrad", 1, (1, 127, 128, 512), 8), ("dgrad", 2, (1, 127, 128, 512), 8), ("dgrad", 2, (1, 63, 128, 512), 4),
        ("wgrad", 1, (1, 63, 64, 512), 8), ("wgrad", 2, (1, 125, 128, 512), 8)]


def _strip_height(kernel, stride, shape):
    """dw_geom's rule (csrc/pool.hip), restated: the rows of the map the kernel's columns belong to."""
    n, h, w, c = shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    rows, cols = (h, w) if kernel == "dgrad" else (ho, wo)
    th = 8
    while th > 2 and n * -(-rows // th) * cols * (c // 4) < (65536 if kernel == "wgrad" else 262144):
        th //= 2
    return th


@pytest.mark.parametrize("kernel,stride,shape,th", TALL)
def test_tall_strips(backend, kernel, stride, shape, th):
    assert _strip_height(kernel, stride, shape) == th and all(_strip_height(k, s, sh) == 2 for sh in GPU_SHAPES + EMU_SHAPES for k in ("fwd", "dgrad", "wgrad") for s in (1, 2))
    n, h, w, c = shape
    g = torch.Generator().manual_seed(41 + stride)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(c, 1, 3, 3, generator=g) / 3.0
    xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, stride, 1, groups=c)
    dy = torch.randn(y.shape, generator=g)
    wk = K.to_dw(wt.to(backend))
    if kernel == "fwd":
        out, parts = K.dwconv3x3_fwd(to_nhwc(x, backend), wk, stride=stride, stat_partials=True)
        assert_close(to_nchw_cpu(out), y.detach().float(), TOL, "dwconv forward")
        assert_close(parts[0].sum(0).cpu(), to_nchw_cpu(out).double().sum((0, 2, 3)).float(), 1e-4, "sum y")
    elif kernel == "dgrad":
        (dx,) = torch.autograd.grad(y, xd, dy.double())
        assert_close(to_nchw_cpu(K.dwconv3x3_bwd_data(to_nhwc(dy, backend), wk, (n, h, w, c), stride=stride)), dx.float(), TOL, "dwconv data gradient")
    else:
        (dw,) = torch.autograd.grad(y, wd, dy.double())
        got = K.dw_empty(c, backend)
        got.zero_()
        K.dwconv3x3_bwd_weight(to_nhwc(x, backend), to_nhwc(dy, backend), got, stride=stride)
        assert_close(got.cpu(), dw.float(), TOL_WGRAD, "dwconv weight gradient")


def _relu6_inputs(backend):
    """Pre-activations that include exactly 0.0 and 6.0 (scale 1, shift 0: the pre-activation is the input, exactly)."""
    n, h, w, c = (2, 9, 7, 32) if backend.type == "cuda" else (1, 3, 2, 16)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, c, h, w, generator=g) * 4.0 + 3.0
    flat = x.view(-1)
    flat[0::7] = 0.0
    flat[3::7] = 6.0
    return x, torch.randn(n, c, h, w, generator=g), c


def test_relu6_affine_act_forward(backend):
    x, _, c = _relu6_inputs(backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    y = K.affine_act(to_nhwc(x, backend), one, zero, act="relu6")
    assert torch.equal(to_nchw_cpu(y), F.relu6(x))
    assert torch.equal(to_nchw_cpu(K.affine_act(to_nhwc(x, backend), act="relu6")), F.relu6(x))


def test_relu6_bn_bwd(backend):
    """BatchNorm + ReLU6 backward (bn_bwd's reduce and apply sweeps): the masked gradient is zero at both ends and dy strictly between,
    and dx / dgamma / dbeta match autograd in fp64 through relu6(batch_norm(x)) with statistics that give scale 1 and shift 0."""
    x, dy, c = _relu6_inputs(backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    dg, db = torch.zeros(c, device=backend), torch.zeros(c, device=backend)
    # scale 1, shift 0, mean 0, invstd 1, gamma 1: y = relu6(x) exactly; bn_bwd differentiates relu6((x - mean) * invstd * gamma + beta)
    dx, g = K.bn_bwd(to_nhwc(dy, backend), to_nhwc(x, backend), one, zero, one, zero, one, dg, db, act="relu6", want_g=True)
    inside = (x > 0) & (x < 6)
    assert torch.equal(to_nchw_cpu(g), torch.where(inside, dy, torch.zeros_like(dy))), "masked gradient: 1 strictly inside (0, 6), 0 at both ends"
    assert bool((to_nchw_cpu(g)[x == 0.0] == 0).all()) and bool((to_nchw_cpu(g)[x == 6.0] == 0).all()) and int((x == 6.0).sum()) > 0
    # autograd in fp64 over the same function with mean / invstd held as the saved statistics' definition requires (mean 0, invstd 1 are inputs
    # here, not statistics of x): dx = g - mean(g) - x * mean(g * x), dgamma = sum g x, dbeta = sum g
    gd, xd = torch.where(inside, dy, torch.zeros_like(dy)).double(), x.double()
    M = x.numel() // c
    sg, sgx = gd.sum((0, 2, 3)), (gd * xd).sum((0, 2, 3))
    ref = gd - (sg / M).view(1, -1, 1, 1) - xd * (sgx / M).view(1, -1, 1, 1)
    assert_close(to_nchw_cpu(dx), ref.float(), TOL, "bn_bwd dx with relu6")
    assert_close(dg.cpu(), sgx.float(), 1e-4, "dgamma")
    assert_close(db.cpu(), sg.float(), 1e-4, "dbeta")
    # and the activation's own derivative against autograd
    xa = x.double().requires_grad_(True)
    (ga,) = torch.autograd.grad(F.relu6(xa), xa, dy.double())
    assert torch.equal(to_nchw_cpu(g).double(), ga)


def _desc(n, h, w, c, k, r, s, stride, pad):
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad = n, h, w, c, k, r, s, stride, pad
    d.Ho, d.Wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    d.x_ld_pix, d.x_ld_img, d.y_ld_pix, d.y_ld_img = c, h * w * c, k, d.Ho * d.Wo * k
    return d


@pytest.mark.parametrize("what,args", [("K != C", dict(k=32)), ("R != 3", dict(r=1, s=1, pad=0)), ("stride 3", dict(stride=3)), ("C % 4 != 0", dict(c=6, k=6))])
def test_rejections(backend, what, args):
    """A bad descriptor is a status with a message from every entry point - never a launch."""
    a = dict(n=1, h=4, w=4, c=16, k=16, r=3, s=3, stride=1, pad=1)
    a.update(args)
    d = _desc(**a)
    L = K.lib()
    buf = torch.zeros(4096, device=backend)
    p = K.ptr(buf)
    assert L.sgx_dwconv3x3_fwd(ctypes.byref(d), p, p, None, p, 0, None, K.stream()) == -1 and L.sgx_last_error()
    assert L.sgx_dwconv3x3_bwd_data(ctypes.byref(d), p, p, p, 0, K.stream()) == -1
    assert L.sgx_dwconv3x3_bwd_weight(ctypes.byref(d), p, p, p, p, buf.numel() * 4, K.stream()) == -1
    assert L.sgx_dwconv3x3_stat_blocks(ctypes.byref(d)) == 0 and L.sgx_dwconv3x3_bwd_weight_workspace(ctypes.byref(d)) == 0
    assert bool((buf == 0).all()), what


def test_relu6_is_rejected_where_it_is_not_implemented(backend):
    n, h, w, c = 1, 4, 4, 16
    g = torch.Generator().manual_seed(1)
    x = to_nhwc(torch.randn(n, c, h, w, generator=g), backend)
    ones = torch.ones(c, device=backend)
    with pytest.raises(_lib.SgxError, match="activation"):
        K.conv2d_fwd(x, K.to_ohwi(torch.randn(c, c, 1, 1, generator=g).to(backend)), act="relu6")
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act(x, ones, ones, act="relu6")
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act(x, ones, ones, x, ones, ones, act="relu6", want_stats=True)
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act_bwd_reduce(x, x, ones, ones, ones, act="relu6")
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act_bwd_reduce(x, x, ones, ones, ones, x, ones, ones, ones, act="relu6")
    # statistics together with bias / activation: rejected by the depthwise forward
    wk = K.to_dw(torch.randn(c, 1, 3, 3, generator=g).to(backend))
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.dwconv3x3_fwd(x, wk, act="relu6", stat_partials=True)
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.dwconv3x3_fwd(x, wk, bias=ones, stat_partials=True)
