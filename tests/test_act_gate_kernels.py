"""The BatchNorm -> activation -> gate sweeps (csrc/se.hip: sgx_bn_act_gate_mean / _fwd / _bwd_gate / _bwd_data) and the gated residual sweep
sgx_bn_gate_add_fwd against plain torch in fp64 and autograd, on the chip and on the host emulation.

Shapes (N, H, W, C), the smallest that cross the boundaries of the sweep skeleton:
  (3, 9, 7, 24)   HW = 63, C4 = 6 (C no multiple of 16): 3 row blocks.  sgx_stats_blocks(189) = 3 gives blocks of exactly 63 rows, so here
                  every block is one image;
  (2, 9, 9, 24)   added for that reason: 3 row blocks of 54 rows against images of 81 pixels - the middle block straddles both images;
  (2, 5, 5, 144)  one row block that holds both images, RL = 7 row lanes;
  (1, 1, 1, 8)    HW = 1, the d = 1 form of the fast division;
  (2, 21, 19, 256) added for the two reductions' own geometry (chunks of 16 rows per row lane: 64 pixels at this width): HW = 399 is six full
                  chunks, whose lanes run the four-rows-in-flight loop, and one of 15 pixels, where three of the four lanes take the tail loop.
The emulation runs (2, 3, 2, 16) only.  Every shape runs contiguous and as channel slices of wider NaN-filled buffers (x_ld > C).

Inputs: pre-activations z span about +-12 (SiLU's whole curved range), a few are planted at +-100, where outputs and gradients must be finite
and, at -100, exactly 0 or -0 (expf overflows to inf: s = 0).  ReLU cases keep z at least KINK from 0.  Bars are the project's: 2e-5 of the
tensor's max-abs for element-wise results (also with the planted elements taken out, so that they do not loosen the bar for the rest), 1e-4
for sums.  Every comparison prints `AG_ERR <kernel> <quantity> <bar> <measured>` before it asserts.
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import test_se_kernels as S
from util import rel_err, to_nchw_cpu

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL, TOL_SUM, KINK, NAN = 2e-5, 1e-4, 1e-3, float("nan")
GPU_SHAPES = [(3, 9, 7, 24), (2, 9, 9, 24), (2, 5, 5, 144), (1, 1, 1, 8), (2, 21, 19, 256)]
EMU_SHAPES = [(2, 3, 2, 16)]
ACTS = {"silu": F.silu, "relu": F.relu, "none": lambda t: t}
GATES = {"sigmoid": torch.sigmoid, "none": lambda p: p}
LAYOUTS = ["slices", "contiguous"]


def _shapes(backend):
    return GPU_SHAPES if backend.type == "cuda" else EMU_SHAPES


def _close(got, ref, tol, kernel, what, keep=None):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"{kernel} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    e = rel_err(got, ref)
    print(f"AG_ERR {kernel} {what} {tol:g} {e:.3e}")
    assert e <= tol, f"{kernel} {what}: max err {e:.3e} of the tensor's max-abs > {tol}"
    if keep is not None and bool(keep.any()) and not bool(keep.all()):  # the same bar without the planted +-100 in the max-abs
        e = rel_err(torch.where(keep, got.double(), 0.0), torch.where(keep, ref.double(), 0.0))
        print(f"AG_ERR {kernel} {what}(unplanted) {tol:g} {e:.3e}")
        assert e <= tol, f"{kernel} {what}: max err {e:.3e} of the unplanted elements' max-abs > {tol}"


def _affine(x, scale, shift):
    return x.double() if scale is None else x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _case(shape, gate, act, affine):
    """Inputs and the fp64 autograd reference of y = f(pre) * act(scale * x + shift), built once and never written afterwards."""
    n, h, w, c = shape
    hw = h * w
    g = torch.Generator().manual_seed(S._seed(n, h, w, c, gate, act, int(affine), "act-gate"))
    pre = torch.randn(n, c, generator=g) * 2.5
    scale = torch.rand(c, generator=g) + 0.5 if affine else None
    shift = torch.randn(c, generator=g) if affine else None
    zt = (torch.rand(n, c, h, w, generator=g) * 2 - 1) * 12.0
    planted = torch.zeros(n, c, h, w, dtype=torch.bool)
    flat, pflat = zt.view(-1), planted.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[: min(6, flat.numel() // 2)]
    flat[where] = torch.tensor([-100.0, 100.0, -100.0, 100.0, -100.0, 100.0])[: where.numel()]
    pflat[where] = True
    if act == "relu":  # away from the kink
        zt = torch.where(zt.abs() < 0.05, zt.sign() * 0.05 + zt, zt)
    x = ((zt - shift.view(1, -1, 1, 1)) / scale.view(1, -1, 1, 1)) if affine else zt.clone()
    z0 = _affine(x, scale, shift)
    assert not (act == "relu" and bool((z0.abs() < KINK).any()))
    assert bool((z0[planted].abs() > 99).all()) and float(z0[~planted].abs().max()) < 13 if bool((~planted).any()) else True
    dy, dmean, mean = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, generator=g), torch.randn(c, generator=g)
    z, pd = z0.clone().requires_grad_(True), pre.double().requires_grad_(True)
    a = ACTS[act](z)
    y = GATES[gate](pd).view(n, c, 1, 1) * a
    gz, gp = torch.autograd.grad(y, (z, pd), dy.double(), retain_graph=True)
    (gz_mean,) = torch.autograd.grad((y * dy.double()).sum() + (a.mean((2, 3)) * dmean.double()).sum(), z)
    return SimpleNamespace(x=x, pre=pre, scale=scale, shift=shift, dy=dy, dmean=dmean, mean=mean, planted=planted, neg=planted & (z0 < 0),
                           a_mean=a.detach().mean((2, 3)), y=y.detach(), gz=gz, gp=gp, gz_mean=gz_mean)


def _zero_at(t_nchw, mask, what):
    if bool(mask.any()):
        assert bool((t_nchw[mask] == 0).all()), f"{what}: not exactly 0 at z = -100: {t_nchw[mask].tolist()}"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "folded"])
@pytest.mark.parametrize("gate", list(GATES))
@pytest.mark.parametrize("act", list(ACTS))
def test_act_gate_sweeps(backend, act, gate, affine, layout):
    """_mean, _fwd, _bwd_gate, _bwd_data (with and without dmean, out of place and over dy) against fp64 autograd; the reduce rows against
    sgx_bn_bwd_reduce on the stored dz, bit for bit; two calls give the same bits; nothing is written outside a channel slice."""
    for shape in _shapes(backend):
        n, h, w, c = shape
        m = n * h * w
        cs = _case(shape, gate, act, affine)
        dev = lambda t: None if t is None else t.to(backend)  # noqa: E731
        pre, scale, shift, dmean, mean = dev(cs.pre), dev(cs.scale), dev(cs.shift), dev(cs.dmean), dev(cs.mean)
        xk, dyk = S._operand(cs.x, backend, layout, 0), S._operand(cs.dy, backend, layout, 1)
        if layout == "slices":
            assert K.rows(xk)[1] > c
        tag = f"{'x'.join(map(str, shape))}/{act}/{gate}/{'affine' if affine else 'folded'}"
        keep = ~cs.planted

        am = K.bn_act_gate_mean(xk, scale, shift, act=act)
        _close(am, cs.a_mean, TOL, "bn_act_gate_mean", f"mean[{tag}]")
        assert S._same_bits(am, K.bn_act_gate_mean(xk, scale, shift, act=act)), "bn_act_gate_mean: a second call gives other bits"

        out = S._result(shape, backend, layout, 2)
        before = S._surround(out)
        assert K.bn_act_gate_fwd(xk, scale, shift, pre, gate, act=act, out=out) is out
        assert torch.equal(S._surround(out), before), "bn_act_gate_fwd wrote outside its channel slice"
        _close(to_nchw_cpu(out), cs.y, TOL, "bn_act_gate_fwd", f"y[{tag}]", keep)
        if act == "silu":
            _zero_at(to_nchw_cpu(out), cs.neg, "bn_act_gate_fwd")
        again = S._result(shape, backend, layout, 3)
        K.bn_act_gate_fwd(xk, scale, shift, pre, gate, act=act, out=again)
        assert S._same_bits(out, again), "bn_act_gate_fwd: a second call gives other bits"

        dpre = K.bn_act_gate_bwd_gate(dyk, xk, scale, shift, pre, gate, act=act)
        _close(dpre, cs.gp, TOL_SUM, "bn_act_gate_bwd_gate", f"dpre[{tag}]")
        assert S._same_bits(dpre, K.bn_act_gate_bwd_gate(dyk, xk, scale, shift, pre, gate, act=act)), "bn_act_gate_bwd_gate: a second call gives other bits"

        dz = S._result(shape, backend, layout, 4)
        before = S._surround(dz)
        _, parts = K.bn_act_gate_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=dz, want_parts=True)
        assert torch.equal(S._surround(dz), before), "bn_act_gate_bwd_data wrote outside its channel slice"
        _close(to_nchw_cpu(dz), cs.gz_mean, TOL, "bn_act_gate_bwd_data", f"dz+dmean[{tag}]", keep)
        plain = S._result(shape, backend, layout, 5)
        K.bn_act_gate_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, out=plain)
        _close(to_nchw_cpu(plain), cs.gz, TOL, "bn_act_gate_bwd_data", f"dz[{tag}]", keep)
        if act == "silu":
            _zero_at(to_nchw_cpu(dz), cs.neg, "bn_act_gate_bwd_data(dmean)")
            _zero_at(to_nchw_cpu(plain), cs.neg, "bn_act_gate_bwd_data")

        assert tuple(parts.shape) == (2, K.stats_blocks(m), c)
        rows = torch.full((2, K.stats_blocks(m), c), NAN, device=backend)
        one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
        K.check(K.lib().sgx_bn_bwd_reduce(K.ptr(dz), K.rows(dz)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(one), K.ptr(zero), K.ptr(mean), m, c, 0, K.ptr(rows),
                                          K.stream()), "sgx_bn_bwd_reduce")
        assert S._same_bits(parts, rows), f"reduce rows differ from bn_bwd_reduce's [{tag}]"
        dzd = to_nchw_cpu(dz).double()
        _close(parts[0].sum(0), dzd.sum((0, 2, 3)), TOL_SUM, "bn_act_gate_bwd_data", f"rows:sum-dz[{tag}]")
        _close(parts[1].sum(0), (dzd * (cs.x.double() - cs.mean.double().view(1, -1, 1, 1))).sum((0, 2, 3)), TOL_SUM, "bn_act_gate_bwd_data", f"rows:sum-dz(x-mean)[{tag}]")

        dz2 = S._result(shape, backend, layout, 6)
        _, parts2 = K.bn_act_gate_bwd_data(dyk, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=dz2, want_parts=True)
        assert S._same_bits(dz, dz2) and S._same_bits(parts, parts2), "bn_act_gate_bwd_data: a second call gives other bits"
        inplace = S._operand(cs.dy, backend, layout, 7)
        before = S._surround(inplace)
        r, parts3 = K.bn_act_gate_bwd_data(inplace, xk, scale, shift, pre, gate, act=act, dmean=dmean, save_mean=mean, out=inplace, want_parts=True)
        assert r is inplace and S._same_bits(inplace, dz) and S._same_bits(parts3, parts), "bn_act_gate_bwd_data(out=dy) differs from the out-of-place call"
        assert torch.equal(S._surround(inplace), before), "bn_act_gate_bwd_data(out=dy) wrote outside its channel slice"


def test_row_blocks_of_the_shapes(backend):
    """What the shapes were chosen for, from the library's own row-block rule."""
    blocks = {s: (K.stats_blocks(s[0] * s[1] * s[2]), -(-s[0] * s[1] * s[2] // K.stats_blocks(s[0] * s[1] * s[2]))) for s in GPU_SHAPES + EMU_SHAPES}
    assert blocks[(3, 9, 7, 24)] == (3, 63) and blocks[(2, 9, 9, 24)] == (3, 54) and blocks[(2, 5, 5, 144)] == (1, 50) and blocks[(1, 1, 1, 8)] == (1, 1) and blocks[(2, 21, 19, 256)] == (13, 62)
    assert blocks[(2, 3, 2, 16)] == (1, 12)
    # the two reductions cut an image into chunks of 16 rows per row lane (256 threads / min(C / 4, 64) lanes), a function of C alone
    for (n, h, w, c), rows in (((3, 9, 7, 24), 672), ((2, 5, 5, 144), 112), ((1, 1, 1, 8), 2048), ((2, 20, 20, 256), 64), ((2, 20, 20, 1152), 64)):
        want = n * -(-h * w // rows) * c * 4 + 256
        assert K.lib().sgx_bn_act_gate_mean_workspace(n, h * w, c) == K.lib().sgx_bn_act_gate_bwd_gate_workspace(n, h * w, c) == want, (n, h, w, c)


@functools.lru_cache(maxsize=None)
def _add_case(shape, gate, affine):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(S._seed(n, h, w, c, gate, int(affine), "gate-add"))
    pre = torch.randn(n, c, generator=g) * 2.5
    scale = torch.rand(c, generator=g) + 0.5 if affine else None
    shift = torch.randn(c, generator=g) if affine else None
    x, r, dy, mean = (torch.randn(n, c, h, w, generator=g) * 3.0, torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g),
                      torch.randn(c, generator=g))
    s = GATES[gate](pre.double()).view(n, c, 1, 1)
    return SimpleNamespace(x=x, r=r, dy=dy, pre=pre, scale=scale, shift=shift, mean=mean, y=s * _affine(x, scale, shift) + r.double(), gz=s * dy.double())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "folded"])
@pytest.mark.parametrize("gate", list(GATES))
def test_bn_gate_add(backend, gate, affine, layout):
    """y = f(pre) * z + r against fp64, out of place and over r; the backward through sgx_bn_gate_act_bwd_data(act none): f(pre) * dy and the
    reduce rows, bit for bit sgx_bn_bwd_reduce's."""
    for shape in _shapes(backend):
        n, h, w, c = shape
        m = n * h * w
        cs = _add_case(shape, gate, affine)
        dev = lambda t: None if t is None else t.to(backend)  # noqa: E731
        pre, scale, shift, mean = dev(cs.pre), dev(cs.scale), dev(cs.shift), dev(cs.mean)
        xk, rk, dyk = S._operand(cs.x, backend, layout, 0), S._operand(cs.r, backend, layout, 1), S._operand(cs.dy, backend, layout, 3)
        tag = f"{'x'.join(map(str, shape))}/{gate}/{'affine' if affine else 'folded'}"
        out = S._result(shape, backend, layout, 2)
        before = S._surround(out)
        assert K.bn_gate_add(xk, scale, shift, pre, gate, rk, out=out) is out
        assert torch.equal(S._surround(out), before), "bn_gate_add wrote outside its channel slice"
        _close(to_nchw_cpu(out), cs.y, TOL, "bn_gate_add_fwd", f"y[{tag}]")
        again = S._result(shape, backend, layout, 4)
        K.bn_gate_add(xk, scale, shift, pre, gate, rk, out=again)
        assert S._same_bits(out, again), "bn_gate_add: a second call gives other bits"
        inplace = S._operand(cs.r, backend, layout, 5)
        before = S._surround(inplace)
        K.bn_gate_add(xk, scale, shift, pre, gate, inplace, out=inplace)
        assert S._same_bits(inplace, out) and torch.equal(S._surround(inplace), before), "bn_gate_add(out=r) differs from the out-of-place call"

        dz = S._result(shape, backend, layout, 6)
        _, parts = K.bn_gate_act_bwd_data(dyk, xk, scale, shift, pre, gate, act="none", save_mean=mean, out=dz, want_parts=True)
        _close(to_nchw_cpu(dz), cs.gz, TOL, "bn_gate_add_fwd", f"backward dz[{tag}]")
        rows = torch.full((2, K.stats_blocks(m), c), NAN, device=backend)
        one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
        K.check(K.lib().sgx_bn_bwd_reduce(K.ptr(dz), K.rows(dz)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(one), K.ptr(zero), K.ptr(mean), m, c, 0, K.ptr(rows),
                                          K.stream()), "sgx_bn_bwd_reduce")
        assert S._same_bits(parts, rows), f"reduce rows differ from bn_bwd_reduce's [{tag}]"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bn_gate_add_dropped_images(backend, layout):
    """Drop-connect's multipliers: gate none, pre[n][:] = 0 or 1 / keep.  A dropped image leaves the residual, bit for bit; a kept one
    matches fp64; the backward of a dropped image is exactly zero."""
    shape = (3, 9, 7, 24) if backend.type == "cuda" else (2, 3, 2, 16)
    n, h, w, c = shape
    cs = _add_case(shape, "none", True)
    mult = torch.tensor([0.0, 1.0 / 0.8, 0.0][:n])
    pre = mult.view(n, 1).expand(n, c).contiguous().to(backend)
    xk, rk, dyk = S._operand(cs.x, backend, layout, 0), S._operand(cs.r, backend, layout, 1), S._operand(cs.dy, backend, layout, 3)
    scale, shift = cs.scale.to(backend), cs.shift.to(backend)
    out = K.bn_gate_add(xk, scale, shift, pre, "none", rk, out=S._result(shape, backend, layout, 2))
    got = to_nchw_cpu(out)
    dropped = mult == 0
    assert torch.equal(got[dropped], cs.r[dropped]), "a dropped image must be the residual itself"
    ref = mult.double().view(n, 1, 1, 1) * _affine(cs.x, cs.scale, cs.shift) + cs.r.double()
    _close(got, ref, TOL, "bn_gate_add_fwd", "drop-connect y")
    dz = K.bn_gate_act_bwd_data(dyk, xk, scale, shift, pre, "none", act="none", out=S._result(shape, backend, layout, 4))
    gz = to_nchw_cpu(dz)
    assert bool((gz[dropped] == 0).all())
    _close(gz, mult.double().view(n, 1, 1, 1) * cs.dy.double(), TOL, "bn_gate_add_fwd", "drop-connect dz")


def test_new_entry_points_reject_unaligned_addresses_and_strides(backend):
    """tests/test_se_kernels.py's scheme on the new entry points: each pointer off by 4 and 8 bytes, each stride off by 2 floats, one defect
    at a time: SGX_ERR_BAD_ARG with a message, and the buffer keeps its bits.  The Python wrappers raise SgxError on the same defects."""
    L, st = K.lib(), K.stream()
    buf = torch.zeros(8192, device=backend)
    base = K.ptr(buf)
    assert base % 16 == 0
    N, C, HW, wsb = 2, 8, 4, 4096 * 4
    R = S._rejections
    tried = R(L, base, "bn_act_gate_mean", lambda **a: L.sgx_bn_act_gate_mean(a["a"], a["a_lp"], a["scale"], a["shift"], 2, a["vec"], N, HW, C, a["ws"], wsb, st),
              ["a", "scale", "shift", "vec", "ws"], ["a_lp"])
    tried += R(L, base, "bn_act_gate_fwd", lambda **a: L.sgx_bn_act_gate_fwd(a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 2, a["o"], a["o_lp"], N, HW, C, 2, st),
               ["a", "o", "scale", "shift", "pre"], ["a_lp", "o_lp"])
    tried += R(L, base, "bn_act_gate_bwd_gate", lambda **a: L.sgx_bn_act_gate_bwd_gate(a["b"], a["b_lp"], a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 2, 2,
                                                                                        a["vec"], N, HW, C, a["ws"], wsb, st),
               ["a", "b", "scale", "shift", "pre", "vec", "ws"], ["a_lp", "b_lp"])
    tried += R(L, base, "bn_act_gate_bwd_data", lambda **a: L.sgx_bn_act_gate_bwd_data(a["b"], a["b_lp"], a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 2, 2,
                                                                                        a["dmean"], a["o"], a["o_lp"], a["mean"], a["parts"], N, HW, C, st),
               ["a", "b", "o", "scale", "shift", "pre", "dmean", "mean", "parts"], ["a_lp", "b_lp", "o_lp"])
    tried += R(L, base, "bn_gate_add_fwd", lambda **a: L.sgx_bn_gate_add_fwd(a["a"], a["a_lp"], a["scale"], a["shift"], a["pre"], 0, a["b"], a["b_lp"], a["o"], a["o_lp"],
                                                                              N, HW, C, st),
               ["a", "b", "o", "scale", "shift", "pre"], ["a_lp", "b_lp", "o_lp"])
    assert tried == 11 + 12 + 16 + 21 + 15
    # workspace too small, scale without shift, unknown codes
    assert L.sgx_bn_act_gate_mean(base, 8, None, None, 2, base + 4096, N, HW, C, base + 8192, 16, st) == -4
    assert L.sgx_bn_act_gate_bwd_gate(base, 8, base, 8, None, None, base + 2048, 2, 2, base + 4096, N, HW, C, base + 8192, 16, st) == -4
    assert L.sgx_bn_act_gate_fwd(base, 8, base + 2048, None, base + 4096, 2, base + 8192, 8, N, HW, C, 2, st) == -1
    assert L.sgx_bn_act_gate_fwd(base, 8, None, None, base + 4096, 7, base + 8192, 8, N, HW, C, 2, st) == -1
    assert L.sgx_bn_act_gate_fwd(base, 8, None, None, base + 4096, 2, base + 8192, 8, N, HW, C, 9, st) == -1
    assert L.sgx_bn_gate_add_fwd(base, 8, None, None, base + 4096, 0, None, 8, base + 8192, 8, N, HW, C, st) == -1
    assert bool((buf.view(torch.int32) == 0).all()), "a rejected call wrote to its buffers"
    x = torch.zeros(1, 2, 2, 18, device=backend)[..., 1:17]  # a channel slice that starts 4 bytes past a 16-byte boundary
    pre = torch.zeros(1, 16, device=backend)
    for call in (lambda: K.bn_act_gate_mean(x, None, None, act="silu"), lambda: K.bn_act_gate_fwd(x, None, None, pre, "sigmoid", act="silu"),
                 lambda: K.bn_act_gate_bwd_gate(x, x, None, None, pre, "sigmoid", act="silu"),
                 lambda: K.bn_act_gate_bwd_data(x, x, None, None, pre, "sigmoid", act="silu"), lambda: K.bn_gate_add(x, None, None, pre, "none", x)):
        with pytest.raises(_lib.SgxError):
            call()
