"""The pool-projection kernels (csrc/inception.h: sgx_pool3_conv1x1_fwd / _bwd_data / _bwd_weight) against plain torch in fp64 -
F.conv2d(F.max_pool2d(x, 3, 1, 1), w) and its autograd, from the same fp32 operands - and the ceil-mode max-pool entry points against
F.max_pool2d(ceil_mode=True), on the chip and on the host emulation of the same sources.  Bars are the project's (tests/test_gconv_kernels.py):
forward and data gradient 2e-5, weight gradient 1e-4, statistics 1e-4 through bn_finalize; the pools are held to equality."""
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import kernels as K

TOL = 2e-5
TOL_WGRAD = 1e-4
# (N, H, W, Ci, Co).  Tiles are 8 rows x 16 columns (8 columns when the map is no wider than 8), chunks of 16 input channels, channel tiles
# of 32 (Co <= 32) or 128 output channels; the data gradient keeps the dy halo tile in LDS up to Co = 156 on 8 x 16 tiles (ic_dg_lds <= 152 KB).
SHAPES = [
    (2, 1, 1, 16, 16),     # every window is mostly padding
    (1, 2, 3, 24, 8),      # a masked last channel chunk, Co below one channel tile
    (2, 7, 7, 40, 36),     # Inception-5's odd map, partial chunk and partial channel tile
    (1, 9, 19, 16, 16),    # several pixel tiles both ways with partial last tiles; the data gradient's halo crosses tile borders
    (2, 14, 14, 48, 144),  # Co > 128: the second channel pass, the weight gradient's third block of 64 (the data gradient: still resident)
]
# data gradient only: Co > 156 on 8 x 16 tiles, the re-read route (158 720 B resident against the 155 648 B limit): dy blocks of 64 / 64 / 32
REREAD = (2, 14, 14, 48, 160)
# weight gradient only: more pixel tiles than workgroups per channel-block pair, so a workgroup walks two tiles.  Chip: 33 tiles of 8 x 8
# against 1024 / (16 x 2 pairs) = 32 workgroups; the emulation caps the split at two workgroups: three tiles.
WALK = {"cuda": (33, 8, 8, 256, 128), "cpu": (3, 3, 3, 16, 16)}
NAN_BITS = torch.tensor(float("nan")).view(torch.int32)
_CASES = {}


def _case(shape, ties=False):
    """Seeded operands and the fp64 reference of one problem (computed once, shared by the tests, never modified).  x = relu(randn) has ties
    at zero in most windows, as in the network; ties=True draws x from {0, 1, 2}: ties everywhere, the selection rule alone decides dx."""
    key = (shape, ties)
    if key not in _CASES:
        n, h, w, ci, co = shape
        g = torch.Generator().manual_seed(41 + 3 * ci + 7 * h + co)
        x = torch.randint(0, 3, (n, ci, h, w), generator=g).float() if ties else torch.relu(torch.randn(n, ci, h, w, generator=g))
        wt = torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5
        bias = torch.randn(co, generator=g) * 0.5
        dy = torch.randn(n, co, h, w, generator=g)
        xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
        y = F.conv2d(F.max_pool2d(xd, 3, 1, 1), wd)
        dx, dw = torch.autograd.grad(y, (xd, wd), dy.double())
        _CASES[key] = dict(x=x, w=wt, bias=bias, y=y.detach(), dy=dy, dx=dx, dw=dw)
    return _CASES[key]


def _slice(t, backend):
    """a channel slice, at offset 4, of a buffer 8 channels wider that is filled with NaN guards"""
    return to_nhwc(t, backend, ld_pix=t.shape[1] + 8, c_off=4)


def _guards_intact(*views):
    for v in views:
        b, c = v._base, v.shape[3]
        g = torch.cat([b[..., :4], b[..., 4 + c:]], 3).cpu().contiguous().view(torch.int32)
        if not bool((g == NAN_BITS).all()):
            return False
    return True


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_forward(backend, i, epilogue):
    n, h, w, ci, co = SHAPES[i]
    fx = _case(SHAPES[i])
    x, wk = _slice(fx["x"], backend), fx["w"].to(backend)
    bias = fx["bias"].to(backend) if epilogue else None
    want = F.relu(fx["y"] + fx["bias"].double().view(1, -1, 1, 1)) if epilogue else fx["y"]
    out = empty_nhwc(n, h, w, co, backend, ld_pix=co + 8, c_off=4)
    y = K.pool3_conv1x1_fwd(x, wk, bias=bias, act="relu" if epilogue else None, out=out)
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), want.float(), TOL, "act(conv1x1(maxpool3(x)) + bias)")
    again = K.pool3_conv1x1_fwd(x, wk, bias=bias, act="relu" if epilogue else None)
    assert torch.equal(to_nchw_cpu(again), to_nchw_cpu(y)), "two calls differ"
    assert _guards_intact(x, out)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_statistics_rows(backend, i):
    n, h, w, ci, co = SHAPES[i]
    fx = _case(SHAPES[i])
    x, wk = _slice(fx["x"], backend), fx["w"].to(backend)
    y, parts = K.pool3_conv1x1_fwd(x, wk, stat_partials=True)
    assert tuple(parts.shape) == (2, K.lib().sgx_pool3_conv1x1_stat_blocks(n, h, w), co)
    assert torch.equal(to_nchw_cpu(y), to_nchw_cpu(K.pool3_conv1x1_fwd(x, wk))), "the statistics output changes what is stored"
    stored, M = to_nchw_cpu(y).double(), n * h * w
    one, zero = torch.ones(co, device=backend), torch.zeros(co, device=backend)
    _, _, mean, invstd = K.bn_finalize(parts, M, one, zero, 1e-5, 0.1, zero.clone(), one.clone())
    assert_close(mean.cpu().double(), stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
    assert_close(1.0 / invstd.cpu().double() ** 2 - 1e-5, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
    assert torch.equal(K.pool3_conv1x1_fwd(x, wk, stat_partials=True)[1].cpu(), parts.cpu()), "statistics rows differ between two calls"


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("i", list(range(len(SHAPES))) + ["ties", "reread"])
def test_data_gradient(backend, i, accumulate):
    shape = SHAPES[3] if i == "ties" else REREAD if i == "reread" else SHAPES[i]
    n, h, w, ci, co = shape
    fx = _case(shape, ties=i == "ties")
    x, dy, wk = _slice(fx["x"], backend), _slice(fx["dy"], backend), fx["w"].to(backend)
    base = torch.randn(n, ci, h, w, generator=torch.Generator().manual_seed(3)) if accumulate else torch.zeros(n, ci, h, w)
    runs = []
    for _ in range(2):
        out = _slice(base, backend)
        dx = K.pool3_conv1x1_bwd_data(dy, wk, x, out=out, accumulate=accumulate)
        assert dx.data_ptr() == out.data_ptr() and _guards_intact(x, dy, out)
        runs.append(to_nchw_cpu(dx))
    assert_close(runs[0], (fx["dx"] + base.double()).float(), TOL, "data gradient through the recomputed arg-max")
    assert torch.equal(runs[0], runs[1]), "two calls differ"


@pytest.mark.parametrize("i", list(range(len(SHAPES))) + ["walk"])
def test_weight_gradient(backend, i):
    """Added onto a non-zero dw; a second call on the same operands gives the same bits."""
    shape = WALK[backend.type] if i == "walk" else SHAPES[i]
    n, h, w, ci, co = shape
    fx = _case(shape)
    x, dy = _slice(fx["x"], backend), _slice(fx["dy"], backend)
    base = torch.randn(co, ci, 1, 1, generator=torch.Generator().manual_seed(5))
    runs = []
    for _ in range(2):
        dw = base.clone().to(backend)
        K.pool3_conv1x1_bwd_weight(x, dy, dw)
        runs.append(dw.cpu())
    assert_close(runs[0] - base, fx["dw"].float(), TOL_WGRAD, "weight gradient")
    assert torch.equal(runs[0], runs[1]), "two calls differ"
    assert _guards_intact(x, dy)


@pytest.mark.parametrize("what,dims,off,null", [("Ci % 4", dict(ci=18), 0, False), ("Co % 4", dict(co=18), 0, False), ("8-byte pointer", {}, 8, False),
                                                ("NULL operand", {}, 0, True), ("H = 0", dict(h=0), 0, False)])
def test_refusals(backend, what, dims, off, null):
    """SGX_ERR_BAD_ARG from every entry point, a message, and nothing written."""
    a = dict(n=1, h=4, w=4, ci=16, co=16)
    a.update(dims)
    dims5 = (a["n"], a["h"], a["w"], a["ci"], a["co"])
    L = K.lib()
    buf = torch.full((8192,), 7.0, device=backend)
    p = K.ptr(buf)
    bad = None if null else p + off
    xs, ys = (a["ci"], 16 * a["ci"]), (a["co"], 16 * a["co"])
    assert L.sgx_pool3_conv1x1_fwd(*dims5, bad, *xs, p, None, p, *ys, 0, None, K.stream()) == -1 and L.sgx_last_error()
    assert L.sgx_pool3_conv1x1_bwd_data(*dims5, p, *ys, p, bad, *xs, p, *xs, 0, K.stream()) == -1
    assert L.sgx_pool3_conv1x1_bwd_weight(*dims5, bad, *xs, p, *ys, p, p, buf.numel() * 4, K.stream()) == -1
    assert bool((buf == 7.0).all()), what


# (k, stride, pad) x (H, W).  3/2/0 and 2/2/0 are GoogLeNet's; ceil and floor extents differ at 4 -> 2 (3/2), 8 -> 4, 6 -> 3 (3/2) and
# 5 -> 3, 7 -> 4 (2/2).  Without padding and with k >= stride the last window always starts inside the map; 2/2/1 is there for the
# "last window starts outside" rule: 5 -> 3 (not 4) and 7 -> 4 (not 5).
@pytest.mark.parametrize("hw,extents", [((2, 3), {(3, 2, 0): (1, 1), (2, 2, 0): (1, 2), (2, 2, 1): (2, 2)}),  # (a map smaller than the 3-window: one clipped window)
                                        ((4, 4), {(3, 2, 0): (2, 2), (2, 2, 0): (2, 2), (2, 2, 1): (3, 3)}),
                                        ((5, 7), {(3, 2, 0): (2, 3), (2, 2, 0): (3, 4), (2, 2, 1): (3, 4)}),
                                        ((8, 6), {(3, 2, 0): (4, 3), (2, 2, 0): (4, 3), (2, 2, 1): (5, 4)})])
@pytest.mark.parametrize("ksp", [(3, 2, 0), (2, 2, 0), (2, 2, 1)])
def test_ceil_mode_pools_equal_aten(backend, ksp, hw, extents):
    k, s, pad = ksp
    g = torch.Generator().manual_seed(11 + k + hw[0])
    x = torch.randint(-3, 4, (2, 8, *hw), generator=g).float().requires_grad_(True)  # (ties; integer dy below: window sums are exact)
    want = F.max_pool2d(x, k, s, pad, ceil_mode=True)
    assert tuple(want.shape[2:]) == extents[ksp]
    dy = torch.randint(-4, 5, want.shape, generator=g).float()
    (dx_want,) = torch.autograd.grad(want, x, dy)
    xs = _slice(x.detach(), backend)
    y, am = K.maxpool_fwd(xs, k, s, pad, ceil_mode=True)
    assert torch.equal(to_nchw_cpu(y), want.detach())
    base = torch.ones(2, 8, *hw)
    out = _slice(base, backend)
    K.maxpool_bwd(_slice(dy, backend), am, tuple(xs.shape), k, s, pad, out=out, accumulate=True, ceil_mode=True)
    assert torch.equal(to_nchw_cpu(out), dx_want + base) and _guards_intact(xs, out)
    assert torch.equal(to_nchw_cpu(K.maxpool_bwd(to_nhwc(dy, backend), am, tuple(xs.shape), k, s, pad, ceil_mode=True)), dx_want)
