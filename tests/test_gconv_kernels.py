"""The grouped 3x3 kernels (csrc/gconv.h: sgx_gconv3x3_fwd / _bwd_data / _bwd_weight) against plain torch in fp64 (F.conv2d(groups=G,
padding=1) and autograd), on the chip and on the host emulation of the same sources.  Bars are the project's: forward and data gradient
2e-5, weight gradient 1e-4, statistics 1e-4 through bn_finalize."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5
TOL_WGRAD = 1e-4
ACTS = {"relu": F.relu, "silu": F.silu, None: lambda t: t}
# (N, H, W, cg, G) and the boundary each is there for.  The kernel's tiles are 16 output channels x (8 or 16 columns: 16 when the map is wider
# than 8) x (64 positions when the whole map has no more, else 128); below 16 channels per group a channel tile spans 16 / cg groups.
GPU_SHAPES = [
    (2, 1, 1, 8, 3),       # map smaller than the window; C = 24: the second channel tile is half outside C
    (1, 2, 2, 16, 3),      # map smaller than the window, one tile per group
    (2, 7, 5, 4, 32),      # odd extents under stride 2 (parity classes of different sizes), four groups per channel tile
    (2, 7, 5, 8, 19),      # odd group count: C = 152, the last channel tile holds ONE group
    (3, 23, 19, 8, 47),    # several position tiles in both directions (3 x 2 of 8 x 16), partial last tiles, odd group count
    (2, 14, 14, 16, 20),   # regnetY800 stage 2
    (2, 9, 9, 32, 5),      # odd extent, two channel tiles and two reduction chunks per group; 8-column tiles at stride 2
    (2, 8, 8, 64, 3),      # cg = 64: four channel tiles, four chunks; exactly 64 positions (the small tile, full)
    (1, 3, 10, 8, 3),      # 16-column tiles with 64 positions (4 rows): a map wider than 8 with at most 64 pixels
    (1, 12, 7, 4, 5),      # 8-column tiles with 128 positions (16 rows): a narrow map with more than 64 pixels; C = 20
    (9, 8, 8, 64, 8),      # weight gradient: MORE position tiles (9) than workgroups per channel-block pair (1024 / 128 pairs = 8), so a
                           # workgroup walks two tiles (re-staging, accumulating across them) and the last one walks one
    (33, 8, 8, 8, 64),     # the same below 16 channels per group: 33 tiles against 1024 / 32 channel blocks = 32 workgroups
]
# the emulation caps the weight gradient at two workgroups per pair: (3, 3, 3, 8, 3) has three tiles, so the first workgroup walks two
EMU_SHAPES = [(2, 5, 3, 8, 3), (1, 2, 2, 4, 5), (2, 3, 3, 16, 2), (3, 3, 3, 8, 3)]
N_SHAPES = max(len(GPU_SHAPES), len(EMU_SHAPES))


def _shape(backend, i):
    shapes = GPU_SHAPES if backend.type == "cuda" else EMU_SHAPES
    return shapes[i % len(shapes)]


_CASES = {}


def _case(shape, stride):
    """Seeded operands and the fp64 reference of one problem (computed once, shared by the tests, never modified)."""
    key = (shape, stride)
    if key not in _CASES:
        n, h, w, cg, G = shape
        c = cg * G
        g = torch.Generator().manual_seed(23 + 31 * stride + c + 7 * h)
        x = torch.randn(n, c, h, w, generator=g)
        wt = torch.randn(c, cg, 3, 3, generator=g) / (3.0 * cg ** 0.5)
        bias = torch.randn(c, generator=g) * 0.5
        xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
        y = F.conv2d(xd, wd, None, stride, 1, groups=G)
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


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_forward_and_statistics_rows(backend, i, stride, strided):
    """The stored y (into a given out); the [2][sgx_gconv3x3_stat_blocks][C] rows of it through bn_finalize; the same bits on a second call."""
    shape = _shape(backend, i)
    n, h, w, cg, G = shape
    c = cg * G
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    wk = K.to_ohwi(fx["w"].to(backend))
    ho, wo = fx["y"].shape[2:]
    out = empty_nhwc(n, ho, wo, c, backend, **_strided(strided, c))
    y = K.gconv3x3_fwd(x, wk, G, out=out, stride=stride)
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), fx["y"].float(), TOL, "grouped 3x3 forward")
    y2, parts = K.gconv3x3_fwd(x, wk, G, stride=stride, stat_partials=True)
    d = K.conv_desc(x, c, 3, 3, stride, 1, y2)
    assert tuple(parts.shape) == (2, K.lib().sgx_gconv3x3_stat_blocks(d.ref, G), c)
    assert torch.equal(to_nchw_cpu(y2), to_nchw_cpu(y)), "the statistics output changes what is stored"
    stored = to_nchw_cpu(y2).double()
    M = stored.shape[0] * stored.shape[2] * stored.shape[3]
    assert_close(parts[0].sum(0).cpu(), stored.sum((0, 2, 3)).float(), 1e-4, "sum y")
    assert_close(parts[1].sum(0).cpu(), (stored * stored).sum((0, 2, 3)).float(), 1e-4, "sum y^2")
    if M > 1:
        mean, var = _finalized(parts, M, backend)
        assert_close(mean, stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
        assert_close(var, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
    _, again = K.gconv3x3_fwd(x, wk, G, stride=stride, stat_partials=True)
    assert torch.equal(parts.cpu(), again.cpu()), "statistics rows differ between two calls"


@pytest.mark.parametrize("act", ["relu", "silu", None])
@pytest.mark.parametrize("stride", [1, 2])
def test_forward_bias_act_epilogue(backend, stride, act):
    shape = _shape(backend, 4)  # (chip: 3 x 23 x 19, cg 8, G 47; emulation: 2 x 5 x 3, cg 8, G 3)
    n, h, w, cg, G = shape
    fx = _case(shape, stride)
    pre = fx["y"] + fx["bias"].double().view(1, -1, 1, 1)
    assert bool((pre > 0.1).any()) and bool((pre < -0.1).any())  # pre-activations on both sides of 0
    y = K.gconv3x3_fwd(to_nhwc(fx["x"], backend), K.to_ohwi(fx["w"].to(backend)), G, bias=fx["bias"].to(backend), act=act, stride=stride)
    assert_close(to_nchw_cpu(y), ACTS[act](pre).float(), TOL, f"act(gconv + bias), {act}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_data_gradient(backend, i, stride, strided):
    shape = _shape(backend, i)
    n, h, w, cg, G = shape
    c = cg * G
    fx = _case(shape, stride)
    dy = to_nhwc(fx["dy"], backend, **_strided(strided, c))
    wk = K.to_ohwi(fx["w"].to(backend))
    out = empty_nhwc(n, h, w, c, backend, **_strided(strided, c))
    dx = K.gconv3x3_bwd_data(dy, wk, G, (n, h, w, c), stride=stride, out=out)
    assert dx.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(dx), fx["dx"].float(), TOL, "grouped 3x3 data gradient")
    base = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(3))
    acc = to_nhwc(base.clone(), backend, **_strided(strided, c))
    K.gconv3x3_bwd_data(dy, wk, G, (n, h, w, c), stride=stride, out=acc, accumulate=True)
    assert_close(to_nchw_cpu(acc), (fx["dx"] + base.double()).float(), TOL, "grouped 3x3 data gradient, accumulate")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_weight_gradient(backend, i, stride, strided):
    """Against fp64; twice on a zeroed dw gives twice the gradient (it accumulates); two calls on the same inputs give the same bits."""
    shape = _shape(backend, i)
    n, h, w, cg, G = shape
    c = cg * G
    fx = _case(shape, stride)
    x = to_nhwc(fx["x"], backend, **_strided(strided, c))
    dy = to_nhwc(fx["dy"], backend, **_strided(strided, c))
    dw = K.ohwi_empty(c, cg, 3, 3, backend)
    dw.zero_()
    K.gconv3x3_bwd_weight(x, dy, dw, G, stride=stride)
    once = dw.cpu().clone()
    assert_close(once, fx["dw"].float(), TOL_WGRAD, "grouped 3x3 weight gradient")
    K.gconv3x3_bwd_weight(x, dy, dw, G, stride=stride)
    assert_close(dw.cpu(), 2.0 * fx["dw"].float(), TOL_WGRAD, "grouped 3x3 weight gradient, second call accumulates")
    dw2 = K.ohwi_empty(c, cg, 3, 3, backend)
    dw2.zero_()
    K.gconv3x3_bwd_weight(x, dy, dw2, G, stride=stride)
    assert torch.equal(dw2.cpu(), once), "weight gradient differs between two calls"


def _desc(n, h, w, c, k, r, s, stride, pad):
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad = n, h, w, c, k, r, s, stride, pad
    d.Ho, d.Wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    d.x_ld_pix, d.x_ld_img, d.y_ld_pix, d.y_ld_img = c, h * w * c, k, d.Ho * d.Wo * k
    return d


@pytest.mark.parametrize("what,args,groups", [("cg = 2", {}, 8), ("K != C", dict(k=32), 2), ("5x5", dict(r=5, s=5, pad=2), 2), ("stride 3", dict(stride=3), 2),
                                              ("C % G != 0", {}, 3), ("groups = 1", {}, 1), ("cg = 12", dict(c=24, k=24), 2)])
def test_rejections(backend, what, args, groups):
    """A bad descriptor or group count is a status with a message from every entry point - never a launch."""
    a = dict(n=1, h=4, w=4, c=16, k=16, r=3, s=3, stride=1, pad=1)
    a.update(args)
    d = _desc(**a)
    L = K.lib()
    buf = torch.zeros(8192, device=backend)
    p = K.ptr(buf)
    assert L.sgx_gconv3x3_fwd(ctypes.byref(d), groups, p, p, None, p, 0, None, K.stream()) == -1 and L.sgx_last_error()
    assert L.sgx_gconv3x3_bwd_data(ctypes.byref(d), groups, p, p, p, 0, None, 0, K.stream()) == -1
    assert L.sgx_gconv3x3_bwd_weight(ctypes.byref(d), groups, p, p, p, p, buf.numel() * 4, K.stream()) == -1
    assert L.sgx_gconv3x3_stat_blocks(ctypes.byref(d), groups) == 0 and L.sgx_gconv3x3_bwd_weight_workspace(ctypes.byref(d), groups) == 0
    assert bool((buf == 0).all()), what


def test_rejects_unaligned_pointers_short_workspace_and_statistics_with_an_epilogue(backend):
    d = _desc(n=1, h=4, w=4, c=16, k=16, r=3, s=3, stride=1, pad=1)
    L = K.lib()
    buf = torch.zeros(8192, device=backend)
    p = K.ptr(buf)
    assert L.sgx_gconv3x3_fwd(ctypes.byref(d), 2, p + 4, p, None, p, 0, None, K.stream()) == -1
    assert L.sgx_gconv3x3_bwd_data(ctypes.byref(d), 2, p, p + 8, p, 0, None, 0, K.stream()) == -1
    assert L.sgx_gconv3x3_bwd_weight(ctypes.byref(d), 2, p, p, p + 4, p, buf.numel() * 4, K.stream()) == -1
    need = L.sgx_gconv3x3_bwd_weight_workspace(ctypes.byref(d), 2)
    assert need > 0 and L.sgx_gconv3x3_bwd_weight(ctypes.byref(d), 2, p, p, p, p, need - 4, K.stream()) == -4
    assert L.sgx_gconv3x3_fwd(ctypes.byref(d), 2, p, p, None, p, 3, None, K.stream()) == -1, "relu6 is not built for this entry point"
    assert bool((buf == 0).all())
    x = to_nhwc(torch.randn(1, 16, 4, 4, generator=torch.Generator().manual_seed(1)), backend)
    wk = K.to_ohwi(torch.randn(16, 8, 3, 3, generator=torch.Generator().manual_seed(2)).to(backend))
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.gconv3x3_fwd(x, wk, 2, act="relu", stat_partials=True)
    with pytest.raises(_lib.SgxError, match="statistics"):
        K.gconv3x3_fwd(x, wk, 2, bias=torch.ones(16, device=backend), stat_partials=True)
