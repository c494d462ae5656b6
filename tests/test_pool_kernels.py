"""The pooling kernels (csrc/pool.hip: sgx_maxpool_fwd / _bwd and their five fp32 kernels, sgx_avgpool_fwd / _bwd; csrc/half.hip:
sgx_hmaxpool_fwd) against ATen on the CPU in fp64, on the chip and on the host emulation of the same sources.

Every comparison is an equality.  The inputs make that possible: x is a multiple of 0.5 in [-1.5, 1.5] (ties in every window, so ATen's
"first maximum in row-major window order" rule is what the arg-max is held to; bf16-exact), gradients and accumulate targets are multiples of
1/256 in [-4, 4] (any sum of up to 169 window terms and a base is below 170 * 4 * 256 < 2^24 units: exact in fp32 in any order).
Every max-pool case names the kernel form the selector is meant to choose for it and asserts that first (K.maxpool_form), so that a later
change of the selector cannot leave a kernel without a test.  Sliced runs read and write channel slices of wider NaN-filled buffers - what
the SPP blocks do with their concat buffers - and check that nothing but the slice was written."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5  # (tests/test_kernels.py's bar; used once, for fp32 sums of randn terms against fp64 - everything else here is exact)
DIRECT, TILE, SCATTER = 0, 1, 2
HALF = torch.bfloat16

# (n, h, w, c, k, stride, pad), forward form, backward form
CASES = [
    ((2, 7, 6, 8, 5, 1, 2), TILE, TILE),
    ((2, 7, 6, 12, 5, 1, 2), DIRECT, DIRECT),
    ((2, 6, 5, 32, 5, 1, 2), TILE, SCATTER),
    ((2, 6, 7, 64, 13, 1, 6), TILE, SCATTER),    # a window larger than the map
    ((2, 9, 8, 8, 3, 2, 1), DIRECT, DIRECT),     # ResNet's stem pool
    ((2, 9, 8, 32, 3, 2, 1), DIRECT, SCATTER),
    ((2, 9, 8, 4, 3, 2, 1), DIRECT, DIRECT),
    ((2, 9, 8, 8, 5, 1, 0), TILE, TILE),         # Wo != W: s_v / s_q are [H * Wo]
    ((2, 9, 8, 8, 5, 1, 1), TILE, TILE),
    ((2, 9, 8, 32, 5, 1, 1), TILE, SCATTER),
    ((1, 8, 9, 8, 2, 2, 0), DIRECT, DIRECT),     # k = 2
    ((1, 8, 9, 32, 2, 2, 0), DIRECT, SCATTER),
    ((1, 8, 9, 8, 2, 1, 1), DIRECT, DIRECT),     # k = 2, Ho = H + 1
    ((1, 5, 5, 8, 3, 3, 0), DIRECT, DIRECT),     # stride 3: rows and columns no window covers get a zero gradient
    ((1, 3, 3, 8, 13, 1, 6), TILE, TILE),
    ((1, 1, 1, 32, 5, 1, 2), TILE, SCATTER),     # a one-pixel map
    ((1, 28, 29, 8, 3, 1, 1), TILE, TILE),       # forward tile form at 64960 B of LDS
    ((1, 29, 29, 8, 3, 1, 1), DIRECT, TILE),     # 67280 B: just past the forward tile limit
    ((1, 35, 39, 8, 3, 1, 1), DIRECT, TILE),     # backward tile form at 65520 B
    ((1, 37, 37, 8, 3, 1, 1), DIRECT, DIRECT),   # 65712 B: just past the backward tile limit
    ((1, 32, 38, 32, 5, 1, 2), DIRECT, SCATTER),  # 155648 B: exactly the scatter form's raised limit
    ((1, 33, 37, 32, 5, 1, 2), DIRECT, TILE),    # one step past it, with C % 32 == 0
    # the first window row reaches row 2 of a 4-row map: a direct backward that walks one output row too far meets image 1's arg-max there
    ((2, 4, 5, 12, 5, 1, 2), DIRECT, DIRECT),
]


def _dyadic(shape, g):
    return torch.randint(-1024, 1025, shape, generator=g).float() / 256.0


def _pool_input(n, c, h, w, g):
    x = torch.randint(-3, 4, (n, c, h, w), generator=g).float() * 0.5
    x[0, 0, :3, :3] = float("-inf")  # windows that hold nothing else: the first element wins, as in ATen
    return x


_REFS = {}


def _ref(case):
    """Seeded operands and the fp64 ATen results of one problem (computed once, shared by the tests, never modified)."""
    if case not in _REFS:
        n, h, w, c, k, s, p = case
        g = torch.Generator().manual_seed(1000 * h + 100 * w + 10 * c + k + s + p)
        x = _pool_input(n, c, h, w, g)
        xd = x.double().requires_grad_(True)
        y, idx = F.max_pool2d(xd, k, s, p, return_indices=True)
        dy = _dyadic(tuple(y.shape), g)
        (dx,) = torch.autograd.grad(y, xd, dy.double())
        base = _dyadic((n, c, h, w), g)
        _REFS[case] = dict(x=x, y=y.detach().float(), idx=idx.to(torch.int32), dy=dy, dx=dx.float(), base=base, acc=(base.double() + dx).float())
    return _REFS[case]


def _assert_forms(case, fwd, bwd):
    n, h, w, c, k, s, p = case
    assert K.maxpool_form(h, w, c, k, s, p) == fwd, f"{case}: the forward selector no longer takes form {fwd}"
    assert K.maxpool_form(h, w, c, k, s, p, backward=True) == bwd, f"{case}: the backward selector no longer takes form {bwd}"


class _Margins:
    """The wide buffer a channel-slice view lives in: its bits outside the slice, taken before a kernel writes the slice."""

    def __init__(self, view, c_off):
        self.buf = view._base
        assert self.buf is not None and self.buf.shape[-1] > view.shape[-1]
        self.outside = torch.ones(self.buf.shape[-1], dtype=torch.bool)
        self.outside[c_off:c_off + view.shape[-1]] = False
        self.before = self._bits()

    def _bits(self):
        b = self.buf.detach().cpu()
        return b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)[..., self.outside].clone()

    def check(self, what, nan=True):
        after = self.buf.detach().cpu()[..., self.outside]
        assert not nan or bool(after.isnan().all()), f"{what}: the kernel wrote outside its channel slice"
        assert torch.equal(self._bits(), self.before), f"{what}: the buffer changed outside the channel slice"


def _views(sliced, c):
    """ld_pix / c_off of x, y, dy and dx (every offset a multiple of 4 floats); {} = contiguous"""
    if not sliced:
        return {}, {}, {}, {}
    return dict(ld_pix=3 * c + 4, c_off=4), dict(ld_pix=2 * c + 8, c_off=c + 4), dict(ld_pix=2 * c + 4, c_off=c), dict(ld_pix=2 * c + 8, c_off=4)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("case,fwd,bwd", CASES, ids=["-".join(map(str, c[0])) for c in CASES])
def test_maxpool_exact(backend, case, fwd, bwd, sliced):
    """y, arg-max, the forward without arg-max, plain and accumulating dx: all equal to ATen's, in every kernel form."""
    _assert_forms(case, fwd, bwd)
    n, h, w, c, k, s, p = case
    r = _ref(case)
    ho, wo = r["y"].shape[2:]
    vx, vy, vdy, vdx = _views(sliced, c)
    margins = []

    def out_buffer(hh, ww, v):
        t = empty_nhwc(n, hh, ww, c, backend, **v)
        if sliced:
            margins.append(_Margins(t, v["c_off"]))
        return t

    x = to_nhwc(r["x"], backend, **vx)
    out = out_buffer(ho, wo, vy)
    y, am = K.maxpool_fwd(x, k, s, p, out=out)
    assert y.data_ptr() == out.data_ptr()
    assert torch.equal(to_nchw_cpu(y), r["y"]), "forward values"
    assert am.dtype == torch.int32 and am.is_contiguous() and torch.equal(to_nchw_cpu(am), r["idx"]), "arg-max: the first maximum in row-major window order"
    out2 = out_buffer(ho, wo, vy)
    y2, none = K.maxpool_fwd(x, k, s, p, out=out2, want_argmax=False)
    assert none is None and torch.equal(to_nchw_cpu(y2), r["y"]), "forward without arg-max"

    dy = to_nhwc(r["dy"], backend, **vdy)
    dxo = out_buffer(h, w, vdx)
    dx = K.maxpool_bwd(dy, am, (n, h, w, c), k, s, p, out=dxo)
    assert dx.data_ptr() == dxo.data_ptr()
    assert torch.equal(to_nchw_cpu(dx), r["dx"]), "dx"
    acc = to_nhwc(r["base"].clone(), backend, **vdx)  # (a clone: on a 1 x 1 map the NHWC view of a CPU tensor is the tensor itself)
    if sliced:
        margins.append(_Margins(acc, vdx["c_off"]))
    K.maxpool_bwd(dy, am, (n, h, w, c), k, s, p, out=acc, accumulate=True)
    assert torch.equal(to_nchw_cpu(acc), r["acc"]), "dx, accumulating"
    for m in margins:
        m.check(f"{case}")
    # the inputs are read only
    assert torch.equal(to_nchw_cpu(x), r["x"]) and torch.equal(to_nchw_cpu(dy), r["dy"]) and torch.equal(to_nchw_cpu(am), r["idx"])


def test_backward_forms_agree_bitwise(backend):
    """csrc/pool.hip says the three backward kernels add a pixel's gradients in the same order (ascending output position, starting from zero):
    on gradients whose sums DO round, the scatter form (32 channels), the tile form (8-channel views) and the direct form (12-channel views)
    must leave the same bits.  (Plain backward only: with `accumulate` the scatter form starts from the target, the gather forms add it last.)"""
    case = (2, 12, 11, 32, 5, 1, 2)
    n, h, w, c, k, s, p = case
    assert K.maxpool_form(h, w, 32, k, s, p, backward=True) == SCATTER and K.maxpool_form(h, w, 8, k, s, p, backward=True) == TILE
    assert K.maxpool_form(h, w, 12, k, s, p, backward=True) == DIRECT
    g = torch.Generator().manual_seed(77)
    x = _pool_input(n, c, h, w, g)
    xd = x.double().requires_grad_(True)
    yr, idx = F.max_pool2d(xd, k, s, p, return_indices=True)
    dy_cpu = torch.randn(tuple(yr.shape), generator=g)
    (ref,) = torch.autograd.grad(yr, xd, dy_cpu.double())
    _, am = K.maxpool_fwd(to_nhwc(x, backend), k, s, p)
    assert torch.equal(to_nchw_cpu(am), idx.to(torch.int32))
    dy = to_nhwc(dy_cpu, backend)
    whole = K.maxpool_bwd(dy, am, (n, h, w, c), k, s, p)
    got = {"scatter": whole}
    for name, cuts in (("tile", (0, 8, 16, 24, 32)), ("direct + tile", (0, 12, 24, 32))):
        dx = torch.full((n, h, w, c), float("nan"), device=backend)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            K.maxpool_bwd(dy[..., lo:hi], am[..., lo:hi].contiguous(), (n, h, w, hi - lo), k, s, p, out=dx[..., lo:hi])  # (arg-max is indexed densely)
        got[name] = dx
    for name, dx in got.items():
        assert torch.equal(dx.cpu(), whole.cpu()), f"the {name} backward differs in bits from the scatter form"
        assert_close(to_nchw_cpu(dx), ref.float(), TOL, f"maxpool backward ({name})")


@pytest.mark.parametrize("c,bwd", [(8, TILE), (12, DIRECT), (32, SCATTER)])
def test_spp_in_buffer(backend, c, bwd):
    """The SPP blocks' use: x and its 5 / 9 / 13 pools are channel slices of ONE concat buffer (the pools read slice 0 and write slices
    1 - 3 of the same allocation); the backward reads slices 1 - 3 of the concat's gradient and accumulates into its slice 0."""
    n, h, w = 2, 9, 8
    ks = (5, 9, 13)
    g = torch.Generator().manual_seed(5 + c)
    x = _pool_input(n, c, h, w, g)
    xd = x.double().requires_grad_(True)
    pools = [F.max_pool2d(xd, k, 1, k // 2) for k in ks]
    dcat_cpu = _dyadic((n, 4 * c, h, w), g)
    grads = [torch.autograd.grad(y, xd, dcat_cpu[:, (i + 1) * c:(i + 2) * c].double())[0] for i, y in enumerate(pools)]
    for k in ks:
        assert K.maxpool_form(h, w, c, k, 1, k // 2) == (TILE if c % 8 == 0 else DIRECT) and K.maxpool_form(h, w, c, k, 1, k // 2, backward=True) == bwd

    cat = torch.full((n, h, w, 4 * c), float("nan"), device=backend)
    cat[..., :c].copy_(x.permute(0, 2, 3, 1).to(backend))
    ams = []
    for i, k in enumerate(ks):
        _, am = K.maxpool_fwd(cat[..., :c], k, 1, k // 2, out=cat[..., (i + 1) * c:(i + 2) * c])
        ams.append(am)
    assert torch.equal(to_nchw_cpu(cat), torch.cat([x.double()] + [y.detach() for y in pools], 1).float()), "x and its three pools in one buffer"

    dcat = to_nhwc(dcat_cpu, backend)
    for i, k in enumerate(ks):
        K.maxpool_bwd(dcat[..., (i + 1) * c:(i + 2) * c], ams[i], (n, h, w, c), k, 1, k // 2, out=dcat[..., :c], accumulate=True)
    after = to_nchw_cpu(dcat)
    assert torch.equal(after[:, :c], (dcat_cpu[:, :c].double() + sum(grads)).float()), "slice 0: its own gradient and the three pools'"
    assert torch.equal(after[:, c:], dcat_cpu[:, c:]), "the gradient slices the pools read have changed"


def _to_nhwc_half(x_nchw, device, ld_pix=None, c_off=0):
    n, c, h, w = x_nchw.shape
    if ld_pix is None:
        return x_nchw.permute(0, 2, 3, 1).contiguous().to(device=device, dtype=HALF)
    buf = torch.full((n, h, w, ld_pix), float("nan"), dtype=HALF, device=device)
    buf[..., c_off:c_off + c].copy_(x_nchw.permute(0, 2, 3, 1).to(device))
    return buf[..., c_off:c_off + c]


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("case", [(2, 7, 6, 8, 5, 1, 2), (2, 9, 8, 24, 3, 2, 1), (2, 9, 8, 8, 5, 1, 0), (1, 3, 3, 16, 13, 1, 6)], ids=lambda c: "-".join(map(str, c)))
def test_maxpool_bf16(backend, case, sliced):
    """hmaxpool_kernel on bf16-exact values (the -inf patch included): the fp32 kernels' result, and ATen's, cast to bf16."""
    n, h, w, c, k, s, p = case
    r = _ref(case)
    assert torch.equal(r["x"].to(HALF).float(), r["x"])
    y32, _ = K.maxpool_fwd(to_nhwc(r["x"], backend), k, s, p, want_argmax=False)
    ho, wo = r["y"].shape[2:]
    x = _to_nhwc_half(r["x"], backend, **(dict(ld_pix=2 * c + 8, c_off=8) if sliced else {}))
    out, margins = None, None
    if sliced:
        out = _to_nhwc_half(torch.full((n, c, ho, wo), float("nan")), backend, ld_pix=c + 16, c_off=8)
        margins = _Margins(out, 8)
    y, none = K.maxpool_fwd(x, k, s, p, out=out, want_argmax=False)
    assert none is None and y.dtype == HALF and (out is None or y.data_ptr() == out.data_ptr())
    assert torch.equal(y.cpu(), y32.cpu().to(HALF)), "bf16 forward against the fp32 kernels"
    assert torch.equal(to_nchw_cpu(y), r["y"].to(HALF)), "bf16 forward against ATen"
    if sliced:
        margins.check(f"bf16 {case}")


@pytest.mark.gpu
def test_direct_kernels_grid_wrap(gpu_device):
    """The direct kernels clamp their grid at 16384 x 256 threads and stride over the rest: 5 x 920 x 920 x 4 is 4 232 000 float4 items against
    4 194 304 threads, forward and backward (ResNet's stem pool wraps from batch 21 backward, from batch 84 forward).  fp32 ATen is reference
    enough: a maximum is exact, and the sums of dyadic gradients are."""
    n, h, w, c, k, s, p = 5, 920, 920, 4, 3, 1, 1
    assert K.maxpool_form(h, w, c, k, s, p) == DIRECT and K.maxpool_form(h, w, c, k, s, p, backward=True) == DIRECT
    assert n * h * w * (c // 4) > 16384 * 256
    g = torch.Generator().manual_seed(9)
    x = _pool_input(n, c, h, w, g).requires_grad_(True)
    yr, idx = F.max_pool2d(x, k, s, p, return_indices=True)
    dy = _dyadic(tuple(yr.shape), g)
    (ref,) = torch.autograd.grad(yr, x, dy)
    y, am = K.maxpool_fwd(to_nhwc(x.detach(), gpu_device), k, s, p)
    assert torch.equal(to_nchw_cpu(y), yr.detach()), "forward values past the grid's first sweep"
    assert torch.equal(to_nchw_cpu(am), idx.to(torch.int32)), "arg-max past the grid's first sweep"
    dx = K.maxpool_bwd(to_nhwc(dy, gpu_device), am, (n, h, w, c), k, s, p)
    assert torch.equal(to_nchw_cpu(dx), ref), "dx past the grid's first sweep"


@pytest.mark.parametrize("shape,sliced", [((2, 7, 7, 8), False), ((2, 7, 7, 8), True), ((2, 1, 1, 8), False), ((1, 3, 5, 12), False)])
def test_avgpool_exact(backend, shape, sliced):
    """The kernels' own arithmetic in high precision: the exact sum (dyadic inputs) times float32(1 / HW), rounded once; dy * float32(1 / HW)."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(3 + h * w + c)
    x = _dyadic((n, c, h, w), g)
    dy = _dyadic((n, c), g)
    inv = float(np.float32(1.0) / np.float32(h * w))
    xd = to_nhwc(x, backend, **(dict(ld_pix=2 * c + 4, c_off=c) if sliced else {}))
    y = K.avgpool_fwd(xd)
    assert tuple(y.shape) == (n, c) and torch.equal(y.cpu(), (x.double().sum((2, 3)) * inv).float()), "avgpool forward"
    dx = K.avgpool_bwd(dy.to(backend), (n, h, w, c))
    assert torch.equal(to_nchw_cpu(dx), (dy.double() * inv).float().view(n, c, 1, 1).expand(n, c, h, w)), "avgpool backward"


@pytest.mark.parametrize("bad", [dict(ld_pix=16, c_off=2), dict(ld_pix=10, c_off=0)], ids=["c_off=2", "ld_pix=10"])
def test_unaligned_views_are_rejected(backend, bad):
    """The kernels move 16-byte channel groups: a view that starts 8 bytes into a pixel, or whose pixels are 40 bytes apart, is a status with a
    message from every pooling entry point - never a launch."""
    n, h, w, c, k = 1, 4, 4, 8, 3
    g = torch.Generator().manual_seed(2)
    x = _pool_input(n, c, h, w, g)
    good = to_nhwc(x, backend)
    y, am = K.maxpool_fwd(good, k, 1, 1)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.maxpool_fwd(to_nhwc(x, backend, **bad), k, 1, 1)
    out = empty_nhwc(n, h, w, c, backend, **bad)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.maxpool_fwd(good, k, 1, 1, out=out)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.maxpool_bwd(to_nhwc(x, backend, **bad), am, (n, h, w, c), k, 1, 1)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.maxpool_bwd(y, am, (n, h, w, c), k, 1, 1, out=out)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.maxpool_bwd(y, am, (n, h, w, c), k, 1, 1, out=out, accumulate=True)
    with pytest.raises(_lib.SgxError, match="16 bytes"):
        K.avgpool_fwd(to_nhwc(x, backend, **bad))
    assert bool(out._base.isnan().all()), "a rejected call wrote its output"
    # (K.avgpool_bwd allocates its own operands: the entry point itself)
    L = K.lib()
    dy, dx = torch.zeros(n, c + 4, device=backend), torch.zeros(n * h * w * (c + 4), device=backend)
    assert L.sgx_avgpool_bwd(n, h * w, c, K.ptr(dy), K.ptr(dx), c, h * w * c, K.stream()) == 0
    dx.zero_()
    assert L.sgx_avgpool_bwd(n, h * w, c, K.ptr(dy) + 8, K.ptr(dx), c, h * w * c, K.stream()) == -1 and b"16 bytes" in L.sgx_last_error()
    assert L.sgx_avgpool_bwd(n, h * w, c, K.ptr(dy), K.ptr(dx) + 8, c, h * w * c, K.stream()) == -1
    assert L.sgx_avgpool_bwd(n, h * w, c, K.ptr(dy), K.ptr(dx), c + 2, h * w * (c + 2), K.stream()) == -1
    assert L.sgx_avgpool_fwd(n, h * w, c, K.ptr(good), c, h * w * c, K.ptr(dy) + 8, K.stream()) == -1
    assert bool((dx == 0).all()) and bool((dy == 0).all())


@pytest.mark.parametrize("h,k,stride", [(3, 5, 1), (4, 5, 2)])
def test_window_larger_than_unpadded_map_is_rejected(backend, h, k, stride):
    """No output position exists (at stride 2 a truncating division would still find one): a status, not a launch."""
    n, c = 1, 8
    x = to_nhwc(_pool_input(n, c, h, h, torch.Generator().manual_seed(4)), backend)
    out = torch.full((n, 1, 1, c), float("nan"), device=backend)
    with pytest.raises(_lib.SgxError, match="empty output"):
        K.maxpool_fwd(x, k, stride, 0, out=out, want_argmax=False)
    dx =torch.full((n, h, h, c), float("nan"), device=backend)
    with pytest.raises(_lib.SgxError, match="empty output"):
        K.maxpool_bwd(torch.zeros(n, 1, 1, c, device=backend), torch.zeros(n, 1, 1, c, dtype=torch.int32, device=backend), (n, h, h, c), k, stride, 0, out=dx)
    assert bool(out.isnan().all()) and bool(dx.isnan().all()), "a rejected call wrote its output"
    assert K.maxpool_form(h, h, c, k, stride, 0) == DIRECT and K.maxpool_form(h, h, c, k, stride, 0, backward=True) == DIRECT
