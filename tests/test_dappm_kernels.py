"""The DAPPM kernels (csrc/dappm.h) against fp64 F.avg_pool2d / F.adaptive_avg_pool2d / F.interpolate(size=...) and their autograd gradients,
on the chip and on the host emulation of the same sources.

Bar, per quantity: ATen's own fp32 CPU result is compared with the same fp64 reference, and the kernel may be 4 x as far (its summation order
differs: separable sums, per-lane partials), with a floor of 1e-6.  Distances are max |a - ref| / max(1, max |ref|): the inputs are randn, so
maps are O(1) and the floor is absolute there; the moment sums grow with the element count, and so does fp32's rounding, hence the scale.
Measured ranges of both errors: DESIGN.md 29.3; the floor decides every case."""
import pytest
import torch
import torch.nn.functional as F

from util import to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

PYRAMID = [(5, 2), (9, 4), (17, 8)]


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1.0))


def _check(got, aten, ref, what):
    e, bar = _err(got, ref), max(4 * _err(aten, ref), 1e-6)
    print(f"{what}: kernel {e:.2e}, ATen fp32 {_err(aten, ref):.2e}")
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all() and e <= bar, f"{what}: {e:.3e} > {bar:.3e}"


def _moments(t):
    return torch.stack([t.sum((0, 2, 3)), (t * t).sum((0, 2, 3))])


def _pyramid_run(x, levels, glob, dys, adds, dtype):
    """ATen in `dtype`: pooled maps, their moments (x's first) and the input gradient for the upstream gradients dys (+ addends)."""
    xd = x.to(dtype).requires_grad_(True)
    outs = [F.avg_pool2d(xd, k, s, s) for k, s in levels] + ([F.adaptive_avg_pool2d(xd, 1)] if glob else [])
    (dx,) = torch.autograd.grad(outs, xd, [d.to(dtype) for d in dys])
    for a in adds:
        dx = dx + a.to(dtype)
    return [o.detach() for o in outs], [_moments(t.detach()) for t in [xd] + outs], dx


# (N, H, W, C), levels, global, x a channel slice, addends + accumulate
CASES = {
    "odd": ((2, 5, 7, 8), PYRAMID, True, False, False),        # odd extents, every window larger than the map
    "workload": ((1, 16, 32, 12), PYRAMID, True, False, False),  # the workload's plane, C a multiple of 4 but not of 8
    "3x3": ((2, 9, 10, 4), PYRAMID, True, False, False),        # the 9 / 4 level ends at 3 x 3
    "tiny": ((1, 3, 3, 8), PYRAMID, True, False, False),        # 17-window output 1 x 1
    "slice": ((2, 5, 7, 8), PYRAMID, True, True, False),
    "single": ((2, 9, 10, 4), [(9, 4)], False, False, False),
    "addends": ((2, 9, 10, 4), PYRAMID, True, False, True),
    # the launch geometries the small cases above never reach (dp_pick_cg widens the channel group only once 512 workgroups exist):
    "cg16": ((4, 5, 7, 2048), PYRAMID, True, False, True),      # CG = 16: four channel lanes, the butterfly starts at lane distance 4
    "cg8": ((4, 10, 6, 1032), PYRAMID, True, False, False),     # CG = 8 (1032 is no multiple of 16)
    "ragged": ((2, 10, 7, 256), PYRAMID, True, False, True),    # backward: 128 workgroups -> four row tiles of 3, 3, 3 and 1 rows
    "lds": ((1, 40, 56, 4), PYRAMID, True, False, False),       # 69 KB of LDS: the forward raises the kernel's dynamic limit
}


@pytest.mark.parametrize("case", list(CASES))
def test_pyramid(backend, case):
    (n, h, w, c), levels, glob, sliced, addends = CASES[case]
    g = torch.Generator().manual_seed(3 + h)
    x = torch.randn(n, c, h, w, generator=g)
    shapes = [(n, c) + K.dappm_pooled_shape(h, w, k, s) for k, s in levels] + ([(n, c, 1, 1)] if glob else [])
    dys = [torch.randn(s, generator=g) for s in shapes]
    adds = [torch.randn(n, c, h, w, generator=g) for _ in range(2)] if addends else []
    base = torch.randn(n, c, h, w, generator=g)
    ref, ref_m, ref_dx = _pyramid_run(x, levels, glob, dys, adds, torch.float64)
    aten, aten_m, aten_dx = _pyramid_run(x, levels, glob, dys, adds, torch.float32)
    xs = to_nhwc(x, backend, **(dict(ld_pix=c + 8, c_off=4) if sliced else {}))
    pooled, parts = K.dappm_pool_fwd(xs, levels, glob)
    assert len(pooled) == len(ref) and len(parts) == len(ref) + 1
    for i, (p, a, r) in enumerate(zip(pooled, aten, ref)):
        _check(to_nchw_cpu(p), a, r, f"{case}: pooled map {i}")
    for i, (p, a, r) in enumerate(zip(parts, aten_m, ref_m)):
        assert p.shape[0] == 2 and p.shape[2] == c
        _check(p.cpu().double().sum(1).float(), a, r, f"{case}: moments of {'x' if i == 0 else f'pooled map {i - 1}'}")
    again, parts2 = K.dappm_pool_fwd(xs, levels, glob)
    assert all(torch.equal(a, b) for a, b in zip(pooled + parts, again + parts2)), "two forward calls differ"

    nl = len(levels)
    args = ([to_nhwc(d, backend) for d in dys[:nl]], levels, (n, h, w, c))
    kw = dict(d_global=to_nhwc(dys[nl], backend) if glob else None, addends=[to_nhwc(a, backend) for a in adds])
    if addends:
        dx = K.dappm_pool_bwd(*args, out=to_nhwc(base.clone(), backend), accumulate=True, **kw)
        dx2 = K.dappm_pool_bwd(*args, out=to_nhwc(base.clone(), backend), accumulate=True, **kw)
        ref_dx, aten_dx = ref_dx + base.double(), aten_dx + base
    else:
        dx, dx2 = K.dappm_pool_bwd(*args, **kw), K.dappm_pool_bwd(*args, **kw)
    _check(to_nchw_cpu(dx), aten_dx, ref_dx, f"{case}: input gradient")
    assert torch.equal(dx, dx2), "two backward calls differ"


# the last three: CG = 16, CG = 8, and forward row tiles of several rows with a ragged last one (10 rows in tiles of 3)
@pytest.mark.parametrize("src,dst,addend,n,c", [(s, d, a, 2, 8) for a in (False, True) for s, d in
                                                 [((2, 3), (5, 7)), ((3, 3), (10, 10)), ((1, 1), (7, 9)), ((4, 8), (16, 32)), ((5, 7), (5, 7))]] +
                         [((2, 3), (5, 7), True, 4, 2048), ((3, 3), (10, 10), True, 4, 1032), ((3, 3), (10, 7), True, 2, 1024)])
def test_resize(backend, src, dst, addend, n, c):
    g = torch.Generator().manual_seed(7 + dst[0])
    z = torch.randn(n, c, *src, generator=g)
    add = torch.randn(n, c, *dst, generator=g) if addend else None
    dy, base = torch.randn(n, c, *dst, generator=g), torch.randn(n, c, *src, generator=g)

    def run(dtype):
        zd = z.to(dtype).requires_grad_(True)
        y = F.interpolate(zd, size=list(dst), mode="bilinear")
        (dz,) = torch.autograd.grad(y, zd, dy.to(dtype))
        y = y.detach() if add is None else y.detach() + add.to(dtype)
        return y, _moments(y), dz

    (ref_y, ref_m, ref_dz), (aten_y, aten_m, aten_dz) = run(torch.float64), run(torch.float32)
    y, parts = K.resize_bilinear_fwd(to_nhwc(z, backend), dst, addend=None if add is None else to_nhwc(add, backend), want_stats=True)
    _check(to_nchw_cpu(y), aten_y, ref_y, "resized map")
    _check(parts.cpu().double().sum(1).float(), aten_m, ref_m, "moments")
    assert torch.equal(K.resize_bilinear_fwd(to_nhwc(z, backend), dst, addend=None if add is None else to_nhwc(add, backend)), y)
    dys = to_nhwc(dy, backend, ld_pix=c + 4, c_off=4)
    dz = K.resize_bilinear_bwd(dys, src)
    _check(to_nchw_cpu(dz), aten_dz, ref_dz, "source gradient")
    assert torch.equal(K.resize_bilinear_bwd(dys, src), dz), "two backward calls differ"
    acc = K.resize_bilinear_bwd(dys, src, out=to_nhwc(base.clone(), backend), accumulate=True)
    _check(to_nchw_cpu(acc), aten_dz + base, ref_dz + base.double(), "source gradient, accumulate")


def test_bad_arguments(backend):
    x = torch.zeros(1, 16, 32, 8, device=backend)
    for levels in ([(19, 8)], PYRAMID + [(5, 2)], [(5, 2, 1)]):  # k = 19, four window levels, another padding
        with pytest.raises(_lib.SgxError):
            K.dappm_pool_fwd(x, levels)
    with pytest.raises(_lib.SgxError):
        K.dappm_pool_fwd(torch.zeros(1, 16, 32, 6, device=backend), PYRAMID)
    with pytest.raises(_lib.SgxError):
        K.resize_bilinear_fwd(torch.zeros(1, 2, 2, 6, device=backend), (4, 4))
