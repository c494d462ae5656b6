"""The depthwise 5x5 kernels (csrc/pool.hip: sgx_dwconv5x5_fwd / _bwd_data / _bwd_weight, both forms of the forward) against plain torch in
fp64 (F.conv2d(groups=C, padding=2) and autograd), on the chip and on the host emulation of the same sources.  Bars as
tests/test_dwconv_kernels.py: forward and data gradient 2e-5, weight gradient 1e-4, statistics 1e-4 through bn_finalize."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5
TOL_WGRAD = 1e-4
HSWISH = lambda t: t * F.relu6(t + 3.0) / 6.0  # noqa: E731
ACTS = {"relu": F.relu, "relu6": F.relu6, "silu": F.silu, "hswish": HSWISH, None: lambda t: t}
# (N, H, W, C): maps smaller than the window (every pixel an edge); odd extents under stride 2, several strips, a channel count that is no
# power of two; even extents; the model's own late layers (several channel tiles)
GPU_SHAPES = [(2, 1, 1, 16), (1, 2, 2, 48), (2, 3, 3, 24), (3, 23, 19, 72), (2, 8, 8, 120), (2, 7, 7, 960), (2, 14, 14, 672)]
EMU_SHAPES = [(2, 5, 3, 16), (1, 2, 2, 48), (2, 1, 1, 16)]
N_SHAPES = max(len(GPU_SHAPES), len(EMU_SHAPES))
FORMS = ["register", "lds"]


def _shape(backend, i):
    shapes = GPU_SHAPES if backend.type == "cuda" else EMU_SHAPES
    return shapes[i % len(shapes)]


_CASES = {}


def _case(shape, stride):
    """Seeded operands and the fp64 reference of one problem (computed once, shared by the tests, never modified)."""
    key = (shape, stride)
    if key not in _CASES:
        n, h, w, c = shape
        g = torch.Generator().manual_seed(19 + 31 * stride + c + 7 * h)
        x = torch.randn(n, c, h, w, generator=g)
        wt = torch.randn(c, 1, 5, 5, generator=g) / 5.0
        bias = torch.randn(c, generator=g) * 0.5
        xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
        y = F.conv2d(xd, wd, None, stride, 2, groups=c)
        dy = torch.randn(y.shape, generator=g)
        dx, dw = torch.autograd.grad(y, (xd, wd), dy.double())
        _CASES[key] = dict(x=x, w=wt, bias=bias, y=y.detach(), dy=dy, dx=dx, dw=dw)
    return _CASES[key]


def _strided(strided, c):
    return dict(ld_pix=c + 8, c_off=4) if strided else {}


def _finalized(parts, M, backend):
    c = parts.shape[2]
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    eps = 1e-5
    _, _, mean, invstd = K.bn_finalize(parts, M, one, zero, eps, 0.1, zero.clone(), one.clone())
    return mean.cpu().double(), 1.0 / invstd.cpu().double() ** 2 - eps


@pytest.fixture
def form(request, backend):
    K.set_dwconv5x5_form(request.param)
    yield request.param
    K.set_dwconv5x5_form("register")


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_forward_and_statistics_rows(backend, form, i, stride, strided):
    """The stored y; the [2][sgx_dwconv5x5_stat_blocks][C] rows of it through bn_finalize; the same bits on a second call."""
    shape = _shape(backend, i)
    n, h, w, c = shape
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    wk = K.to_dw(fx["w"].to(backend))
    ho, wo = fx["y"].shape[2:]
    out = empty_nhwc(n, ho, wo, c, backend, **_strided(strided, c))
    y = K.dwconv5x5_fwd(x, wk, out=out, stride=stride)
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), fx["y"].float(), TOL, "dwconv 5x5 forward")
    y2, parts = K.dwconv5x5_fwd(x, wk, stride=stride, stat_partials=True)
    d = K.conv_desc(x, c, 5, 5, stride, 2, y2)
    assert tuple(parts.shape) == (2, K.lib().sgx_dwconv5x5_stat_blocks(d.ref), c)
    assert torch.equal(to_nchw_cpu(y2), to_nchw_cpu(y)), "the statistics output changes what is stored"
    stored = to_nchw_cpu(y2).double()
    M = stored.shape[0] * stored.shape[2] * stored.shape[3]
    assert_close(parts[0].sum(0).cpu(), stored.sum((0, 2, 3)).float(), 1e-4, "sum y")
    assert_close(parts[1].sum(0).cpu(), (stored * stored).sum((0, 2, 3)).float(), 1e-4, "sum y^2")
    if M > 1:
        mean, var = _finalized(parts, M, backend)
        assert_close(mean, stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
        assert_close(var, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
    _, again = K.dwconv5x5_fwd(x, wk, stride=stride, stat_partials=True)
    assert torch.equal(parts.cpu(), again.cpu()), "statistics rows differ between two calls"


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("act", ["relu", "relu6", "silu", "hswish", None])
@pytest.mark.parametrize("stride", [1, 2])
def test_forward_bias_act_epilogue(backend, form, stride, act):
    shape = _shape(backend, 3)  # (chip: 3 x 23 x 19 x 72; emulation: 2 x 5 x 3 x 16)
    fx = _case(shape, stride)
    pre = fx["y"] * 4.0 + fx["bias"].double().view(1, -1, 1, 1)  # (x 4: pre-activations on both sides of -3, 0, 3 and 6)
    assert all(bool(((pre > lo) & (pre < hi)).any()) for lo, hi in ((-1e9, -3), (-3, 0), (0, 3), (3, 6), (6, 1e9)))
    y = K.dwconv5x5_fwd(to_nhwc(fx["x"], backend), K.to_dw((fx["w"] * 4.0).to(backend)), bias=fx["bias"].to(backend), act=act, stride=stride)
    assert_close(to_nchw_cpu(y), ACTS[act](pre).float(), TOL, f"act(dwconv + bias), {act}")


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
    dx = K.dwconv5x5_bwd_data(dy, wk, (n, h, w, c), stride=stride, out=out)
    assert dx.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(dx), fx["dx"].float(), TOL, "dwconv 5x5 data gradient")
    base = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(3))
    acc = to_nhwc(base.clone(), backend, **_strided(strided, c))
    K.dwconv5x5_bwd_data(dy, wk, (n, h, w, c), stride=stride, out=acc, accumulate=True)
    assert_close(to_nchw_cpu(acc), (fx["dx"] + base.double()).float(), TOL, "dwconv 5x5 data gradient, accumulate")


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
    dw = K.dw_empty(c, backend, 5)
    dw.zero_()
    K.dwconv5x5_bwd_weight(x, dy, dw, stride=stride)
    once = dw.cpu().clone()
    assert_close(once, fx["dw"].float(), TOL_WGRAD, "dwconv 5x5 weight gradient")
    K.dwconv5x5_bwd_weight(x, dy, dw, stride=stride)
    assert_close(dw.cpu(), 2.0 * fx["dw"].float(), TOL_WGRAD, "dwconv 5x5 weight gradient, second call accumulates")
    dw2 = K.dw_empty(c, backend, 5)
    dw2.zero_()
    K.dwconv5x5_bwd_weight(x, dy, dw2, stride=stride)
    assert torch.equal(dw2.cpu(), once), "weight gradient differs between two calls"


# Strip heights (csrc/pool.hip dw_geom at two channels per lane: TH = 8, halved to 2 until a launch has 262 144 threads, 65 536 for the weight
# gradient; the LDS form: TH = 8 at stride 1, 4 at stride 2, halved to 2 until N x strips x column tiles x channel tiles x 256 threads reach
# 262 144).  The shapes above all run TH = 2; these run TH = 8 and TH = 4 with partial last strips.  (kernel, stride, shape, TH)
TALL = [("fwd", 1, (1, 63, 128, 512), 8), ("fwd", 2, (1, 125, 256, 512), 8), ("fwd", 1, (1, 31, 128, 512), 4),
        ("dgrad", 1, (1, 63, 128, 512), 8), ("dgrad", 2, (1, 63, 128, 512), 8), ("dgrad", 2, (1, 31, 128, 512), 4),
        ("wgrad", 1, (1, 31, 64, 512), 8), ("wgrad", 2, (1, 61, 128, 512), 8), ("wgrad", 1, (1, 15, 64, 512), 4),
        ("lds", 1, (4, 63, 64, 512), 8), ("lds", 2, (4, 61, 64, 512), 4)]


def _strip_height(kernel, stride, shape):
    n, h, w, c = shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if kernel == "lds":
        th, tw, ctiles = (8, min(16, wo)) if stride == 1 else (4, min(8, wo)), None, -(-(c // 4) // 8)
        th, tw = th
        while th > 2 and n * -(-ho // th) * -(-wo // tw) * ctiles * 256 < 262144:
            th //= 2
        return th
    rows, cols = (h, w) if kernel == "dgrad" else (ho, wo)
    th = 8
    while th > 2 and n * -(-rows // th) * cols * (c // 2) < (65536 if kernel == "wgrad" else 262144):
        th //= 2
    return th


def test_strip_heights_of_the_small_shapes():
    assert all(_strip_height(k, s, sh) == 2 for sh in GPU_SHAPES + EMU_SHAPES for k in ("fwd", "dgrad", "wgrad", "lds") for s in (1, 2))
    assert all(_strip_height(k, s, sh) == th for k, s, sh, th in TALL)


@pytest.mark.parametrize("kernel,stride,shape,th", TALL)
def test_tall_strips(backend, kernel, stride, shape, th):
    if backend.type != "cuda":
        shape = (1, 11, 8, 16)  # (the emulation walks one fiber per thread: a small map, TH = 2, checks the call path only)
    n, h, w, c = shape
    g = torch.Generator().manual_seed(41 + stride)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(c, 1, 5, 5, generator=g) / 5.0
    xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, stride, 2, groups=c)
    dy = torch.randn(y.shape, generator=g)
    wk = K.to_dw(wt.to(backend))
    if kernel in ("fwd", "lds"):
        K.set_dwconv5x5_form("lds" if kernel == "lds" else "register")
        try:
            out, parts = K.dwconv5x5_fwd(to_nhwc(x, backend), wk, stride=stride, stat_partials=True)
        finally:
            K.set_dwconv5x5_form("register")
        assert_close(to_nchw_cpu(out), y.detach().float(), TOL, "dwconv 5x5 forward")
        assert_close(parts[0].sum(0).cpu(), to_nchw_cpu(out).double().sum((0, 2, 3)).float(), 1e-4, "sum y")
    elif kernel == "dgrad":
        (dx,) = torch.autograd.grad(y, xd, dy.double())
        assert_close(to_nchw_cpu(K.dwconv5x5_bwd_data(to_nhwc(dy, backend), wk, (n, h, w, c), stride=stride)), dx.float(), TOL, "dwconv 5x5 data gradient")
    else:
        (dw,) = torch.autograd.grad(y, wd, dy.double())
        got = K.dw_empty(c, backend, 5)
        got.zero_()
        K.dwconv5x5_bwd_weight(to_nhwc(x, backend), to_nhwc(dy, backend), got, stride=stride)
        assert_close(got.cpu(), dw.float(), TOL_WGRAD, "dwconv 5x5 weight gradient")


def _desc(n, h, w, c, k, r, s, stride, pad):
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad = n, h, w, c, k, r, s, stride, pad
    d.Ho, d.Wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    d.x_ld_pix, d.x_ld_img, d.y_ld_pix, d.y_ld_img = c, h * w * c, k, d.Ho * d.Wo * k
    return d


@pytest.mark.parametrize("what,args", [("K != C", dict(k=32)), ("R = 5 with pad 1", dict(pad=1)), ("R != 5", dict(r=3, s=3, pad=1)), ("stride 3", dict(stride=3)),
                                       ("C % 4 != 0", dict(c=6, k=6))])
def test_rejections(backend, what, args):
    """A bad descriptor is a status with a message from every entry point - never a launch."""
    a = dict(n=1, h=4, w=4, c=16, k=16, r=5, s=5, stride=1, pad=2)
    a.update(args)
    d = _desc(**a)
    L = K.lib()
    buf = torch.zeros(8192, device=backend)
    p = K.ptr(buf)
    assert L.sgx_dwconv5x5_fwd(ctypes.byref(d), p, p, None, p, 0, None, K.stream()) == -1 and L.sgx_last_error()
    assert L.sgx_dwconv5x5_bwd_data(ctypes.byref(d), p, p, p, 0, K.stream()) == -1
    assert L.sgx_dwconv5x5_bwd_weight(ctypes.byref(d), p, p, p, p, buf.numel() * 4, K.stream()) == -1
    assert L.sgx_dwconv5x5_stat_blocks(ctypes.byref(d)) == 0 and L.sgx_dwconv5x5_bwd_weight_workspace(ctypes.byref(d)) == 0
    assert bool((buf == 0).all()), what


def test_rejects_unaligned_pointers_short_workspace_and_statistics_with_an_epilogue(backend):
    d = _desc(n=1, h=4, w=4, c=16, k=16, r=5, s=5, stride=1, pad=2)
    L = K.lib()
    buf = torch.zeros(8192, device=backend)
    p = K.ptr(buf)
    assert L.sgx_dwconv5x5_fwd(ctypes.byref(d), p + 4, p, None, p, 0, None, K.stream()) == -1
    assert L.sgx_dwconv5x5_bwd_data(ctypes.byref(d), p, p + 8, p, 0, K.stream()) == -1
    assert L.sgx_dwconv5x5_bwd_weight(ctypes.byref(d), p, p, p + 4, p, buf.numel() * 4, K.stream()) == -1
    need = L.sgx_dwconv5x5_bwd_weight_workspace(ctypes.byref(d))
    assert need > 0 and L.sgx_dwconv5x5_bwd_weight(ctypes.byref(d), p, p, p, p, need - 4, K.stream()) == -4
    assert L.sgx_dwconv5x5_fwd(ctypes.byref(d), p, p, None, p, 5, None, K.stream()) == -1, "activation code 5 does not exist"
    assert bool((buf == 0).all())
    x = to_nhwc(torch.randn(1, 16, 4, 4, generator=torch.Generator().manual_seed(1)), backend)
    wk = K.to_dw(torch.randn(16, 1, 5, 5, generator=torch.Generator().manual_seed(2)).to(backend))
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.dwconv5x5_fwd(x, wk, act="hswish", stat_partials=True)
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.dwconv5x5_fwd(x, wk, bias=torch.ones(16, device=backend), stat_partials=True)
