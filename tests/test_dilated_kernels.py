"""The split-dilation grouped 3x3 kernels (csrc/dilated.h: sgx_dgconv3x3_fwd / _bwd_data / _bwd_weight) against plain torch in fp64
(F.conv2d(dilation=d, padding=d, groups) per split, concatenated, and autograd), on the chip and on the host emulation of the same sources.
Bars are test_gconv_kernels.py's: forward and data gradient 2e-5, weight gradient 1e-4, statistics 1e-4 through bn_finalize."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gconv_kernels import _desc, _finalized
from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import kernels as K

TOL = 2e-5
TOL_WGRAD = 1e-4
CG = 16
# (C, dilations, (N, H, W), staging form of each split).  Tiles are gconv's: 8 x 16 positions on the 19 x 23 and 9 x 17 maps, 8 x 8 on
# 4 x 5.  Halo while (TH + 2d)(TW + 2d) <= 561: d = 4 is 16 x 24 = 384, d = 14 is 36 x 44; a band wider than three tiles (d > TW) is "tiles".
CASES = [
    (32, (1, 14), (2, 19, 23), ("halo", "band")),   # d = 14 with taps inside and outside the map; 3 x 2 tiles, partial last tiles
    (32, (1, 14), (1, 4, 5), ("halo", "tiles")),    # only the centre tap of the d = 14 split survives
    (64, (1, 4), (2, 9, 17), ("halo", "halo")),
    (48, (1, 2, 3), (2, 9, 17), ("halo",) * 3),     # three splits
    (32, (3,), (2, 9, 17), ("halo",)),              # one split: the single-dilation Conv2d form
    (32, (1, 17), (1, 19, 23), ("halo", "tiles")),  # d above the 16-column tile on a map wider and taller than d: live side taps of "tiles"
]
_REF = {}


def _case(i):
    """Seeded operands and the fp64 reference of one case (computed once, shared by the tests, never modified)."""
    if i not in _REF:
        c, dils, (n, h, w), _ = CASES[i]
        cs = c // len(dils)
        g = torch.Generator().manual_seed(41 + i)
        x = torch.randn(n, c, h, w, generator=g)
        ws = [torch.randn(cs, CG, 3, 3, generator=g) / 12.0 for _ in dils]
        xd, wd = x.double().requires_grad_(True), [t.double().requires_grad_(True) for t in ws]
        y = torch.cat([F.conv2d(xs, wi, None, 1, d, d, cs // CG) for xs, wi, d in zip(xd.split(cs, 1), wd, dils)], 1)
        dy = torch.randn(y.shape, generator=g)
        dx, *dw = torch.autograd.grad(y, [xd] + wd, dy.double())
        _REF[i] = dict(x=x, ws=ws, bias=torch.randn(c, generator=g) * 0.5, y=y.detach(), dy=dy, dx=dx, dw=dw)
    return _REF[i]


def _sliced(i, c):
    return dict(ld_pix=c + 8, c_off=4) if i == 0 else {}  # case 0 runs on channel slices of wider buffers


@pytest.mark.parametrize("i", range(len(CASES)))
def test_forward_statistics_and_form(backend, i):
    c, dils, (n, h, w), forms = CASES[i]
    fx = _case(i)
    assert tuple(K.dgconv3x3_form((n, h, w, c), CG, dils, s) for s in range(len(dils))) == forms
    x = to_nhwc(fx["x"], backend, **_sliced(i, c))
    wk = [K.to_ohwi(t.to(backend)) for t in fx["ws"]]
    out = empty_nhwc(n, h, w, c, backend, **_sliced(i, c))
    y, parts = K.dgconv3x3_fwd(x, wk, CG, dils, out=out, stat_partials=True)
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), fx["y"].float(), TOL, "dilated grouped 3x3 forward")
    d = K.conv_desc(x, c, 3, 3, 1, 1, y)
    assert tuple(parts.shape) == (2, K.lib().sgx_dgconv3x3_stat_blocks(d.ref, CG, len(dils), (ctypes.c_int32 * len(dils))(*dils)), c)
    stored = to_nchw_cpu(y).double()
    mean, var = _finalized(parts, n * h * w, backend)
    assert_close(mean, stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
    assert_close(var, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
    y2, again = K.dgconv3x3_fwd(x, wk, CG, dils, stat_partials=True)
    assert torch.equal(to_nchw_cpu(y2), to_nchw_cpu(y)) and torch.equal(parts.cpu(), again.cpu()), "two calls differ"
    if i == 0:
        pre = fx["y"] + fx["bias"].double().view(1, -1, 1, 1)
        ya = K.dgconv3x3_fwd(x, wk, CG, dils, bias=fx["bias"].to(backend), act="relu")
        assert_close(to_nchw_cpu(ya), F.relu(pre).float(), TOL, "relu(conv + bias)")


@pytest.mark.parametrize("i", range(len(CASES)))
def test_data_gradient(backend, i):
    c, dils, (n, h, w), _ = CASES[i]
    fx = _case(i)
    dy = to_nhwc(fx["dy"], backend, **_sliced(i, c))
    wk = [K.to_ohwi(t.to(backend)) for t in fx["ws"]]
    out = empty_nhwc(n, h, w, c, backend, **_sliced(i, c))
    dx = K.dgconv3x3_bwd_data(dy, wk, CG, dils, out=out)
    assert_close(to_nchw_cpu(dx), fx["dx"].float(), TOL, "dilated grouped 3x3 data gradient")
    assert torch.equal(to_nchw_cpu(K.dgconv3x3_bwd_data(dy, wk, CG, dils)), to_nchw_cpu(dx)), "two calls differ"
    if i == 0:
        base = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(3))
        acc = to_nhwc(base.clone(), backend, **_sliced(i, c))
        K.dgconv3x3_bwd_data(dy, wk, CG, dils, out=acc, accumulate=True)
        assert_close(to_nchw_cpu(acc), (fx["dx"] + base.double()).float(), TOL, "data gradient, accumulate")


@pytest.mark.parametrize("i", range(len(CASES)))
def test_weight_gradient(backend, i):
    """Against fp64; a second call on the same dw doubles it (it accumulates); two calls on the same inputs give the same bits."""
    c, dils, (n, h, w), _ = CASES[i]
    fx = _case(i)
    x = to_nhwc(fx["x"], backend, **_sliced(i, c))
    dy = to_nhwc(fx["dy"], backend, **_sliced(i, c))
    cs = c // len(dils)
    dws = [K.ohwi_empty(cs, CG, 3, 3, backend).zero_() for _ in dils]
    K.dgconv3x3_bwd_weight(x, dy, dws, CG, dils)
    once = [t.cpu().clone() for t in dws]
    for s, t in enumerate(once):
        assert_close(t, fx["dw"][s].float(), TOL_WGRAD, f"weight gradient of split {s}")
    K.dgconv3x3_bwd_weight(x, dy, dws, CG, dils)
    again = [K.ohwi_empty(cs, CG, 3, 3, backend).zero_() for _ in dils]
    K.dgconv3x3_bwd_weight(x, dy, again, CG, dils)
    for s in range(len(dils)):
        assert_close(dws[s].cpu(), 2.0 * fx["dw"][s].float(), TOL_WGRAD, f"split {s}: the second call accumulates")
        assert torch.equal(again[s].cpu(), once[s]), f"split {s}: weight gradient differs between two calls"


@pytest.mark.parametrize("what,cg,dils", [("cg = 8", 8, (1, 2)), ("cg = 24", 24, (1,)), ("5 splits", 16, (1,) * 5), ("0 splits", 16, ()),
                                          ("C % nsplit", 16, (1, 2, 3)), ("dilation 0", 16, (1, 0))])
def test_rejections(backend, what, cg, dils):
    """A bad group width, split count or dilation is a status from every entry point - never a launch."""
    d = _desc(n=1, h=4, w=4, c=64, k=64, r=3, s=3, stride=1, pad=1)
    L = K.lib()
    buf = torch.zeros(16384, device=backend)
    p = K.ptr(buf)
    ns = len(dils)
    dil, wp = (ctypes.c_int32 * max(ns, 1))(*dils), (ctypes.c_void_p * 5)(*([p] * 5))
    assert L.sgx_dgconv3x3_fwd(ctypes.byref(d), cg, ns, dil, wp, p, None, p, 0, None, K.stream()) == -1 and L.sgx_last_error()
    assert L.sgx_dgconv3x3_bwd_data(ctypes.byref(d), cg, ns, dil, p, wp, p, 0, K.stream()) == -1
    assert L.sgx_dgconv3x3_bwd_weight(ctypes.byref(d), cg, ns, dil, p, p, wp, p, buf.numel() * 4, K.stream()) == -1
    assert L.sgx_dgconv3x3_stat_blocks(ctypes.byref(d), cg, ns, dil) == 0 and L.sgx_dgconv3x3_bwd_weight_workspace(ctypes.byref(d), cg, ns, dil) == 0
    assert bool((buf == 0).all()), what
