"""The ShuffleNetV2 kernels of csrc/shuffle.h against plain torch in fp64 on the same fp32 operands:
  sgx_shuffle_merge_fwd          y[:, 2i] = L[:, i], y[:, 2i + 1] = R[:, i]; a side is copied bit for bit or is act(scale * x + shift)
  sgx_shuffle_merge_bwd_reduce   the BatchNorm-backward reduce rows of the affine side(s) from the interleaved gradient (2 or 4 planes)
  sgx_shuffle_merge_bwd_apply    dt of the affine side(s), the copy side's gradient elements bit for bit into its own target
Both back ends (the chip under -m gpu, the host emulation of the same sources otherwise) run the same cases.

Bars (relative, max-norm, against fp64; tests/test_dense_kernels.py): element outputs 2e-5, quantities that went through a finalize (dgamma,
dbeta) 1e-4.  ReLU cases keep every fp64 pre-activation 1e-3 away from 0 (test_bn_kernels._away_from_kinks, through test_dense_kernels._nudged).

Shapes, the smallest that reach each launch form: h in {4, 36, 260} - one channel group; nine groups (28 row lanes, four idle threads); two
256-channel strips - and M in {3, 70, 1024} - fewer rows than row lanes; a remainder behind the unrolled rows; several row blocks.  Every
operand is a channel slice of a buffer 8 channels wider that holds a guard value; `left` sits at a non-zero slice offset.
"""
import pytest
import torch
import torch.nn.functional as F

from super_gradients_amd import kernels as K
from test_dense_kernels import EPS, GUARD, MOM, TOL, TOL_FIN, _bn_affine, _close, _gen, _nudged, _wide

SHAPES = {"M3": (1, 3, 1), "M70": (2, 7, 5), "M1024": (4, 16, 16)}
HS = [4, 36, 260]


class _Side:
    """One affine side: x [n, hh, w, h] (ReLU pre-activations away from 0), its BatchNorm's gamma / beta and the fp32 roundings of the fp64
    training-mode scale, shift, mean, invstd."""

    def __init__(self, g, shape, h, dev):
        n, hh, w = shape
        self.gamma, self.beta = torch.rand(h, generator=g) + 0.5, torch.randn(h, generator=g) * 0.3
        self.x = _nudged(torch.randn(n, hh, w, h, generator=g) * 2.0 + 0.5, self.gamma, self.beta)
        self.scale, self.shift, self.mean, self.invstd = (t.float() for t in _bn_affine(self.x, self.gamma, self.beta))
        self.dev_stats = tuple(t.to(dev) for t in (self.scale, self.shift, self.mean, self.invstd))

    def fwd64(self):
        return F.relu(self.scale.double() * self.x.double() + self.shift.double())

    def bwd64(self, dy):
        """fp64 autograd of training-mode BatchNorm -> ReLU: (dx, dgamma, dbeta, sum g, sum g * (x - mean))"""
        xd, wd, bd = (t.double().requires_grad_(True) for t in (self.x, self.gamma, self.beta))
        y = F.batch_norm(xd.permute(0, 3, 1, 2), None, None, wd, bd, True, MOM, EPS)
        F.relu(y).backward(dy.double().permute(0, 3, 1, 2))
        h = self.x.shape[3]
        gm = (dy.double() * (y.detach().permute(0, 2, 3, 1) > 0)).reshape(-1, h)
        xc = self.x.double().reshape(-1, h)
        return xd.grad, wd.grad, bd.grad, gm.sum(0), (gm * (xc - xc.mean(0))).sum(0)


def _guards_ok(buf, off, c):
    b = buf.cpu()
    return bool((b[..., :off] == GUARD).all()) and bool((b[..., off + c:] == GUARD).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("mode", ["copy_affine", "affine_affine", "copy_copy"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_merge_fwd(backend, shape, h, mode):
    dev = backend
    n, hh, w = SHAPES[shape]
    g = _gen(100 * n * hh + h)
    right = _Side(g, SHAPES[shape], h, dev)
    left = _Side(g, SHAPES[shape], h, dev)
    lx, rx = left.x.clone(), right.x.clone()
    for t in ((lx, rx) if mode == "copy_copy" else (lx,) if mode == "copy_affine" else ()):
        f = t.view(-1)
        f[0], f[1], f[2] = -0.0, 1e-41, float("nan")  # a copy moves bits: the sign of zero, a denormal, a NaN
        f.view(torch.int32)[f.numel() - 1] = 0x7FC12345  # (a NaN with a payload)
    lv, _ = _wide(lx, dev, off=4)
    rv, _ = _wide(rx, dev)
    la = mode == "affine_affine"
    ra = mode != "copy_copy"
    outs = []
    for _ in range(2):
        yv, ybuf = _wide(torch.zeros(n, hh, w, 2 * h), dev, off=4)
        K.shuffle_merge(lv, rv, lscale=left.dev_stats[0] if la else None, lshift=left.dev_stats[1] if la else None, lact="relu" if la else None,
                        rscale=right.dev_stats[0] if ra else None, rshift=right.dev_stats[1] if ra else None, ract="relu" if ra else None, out=yv)
        assert _guards_ok(ybuf, 4, 2 * h), "the forward wrote outside its slice"
        outs.append(yv.cpu().clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "a second call from the same inputs differs"
    y = outs[0]
    for name, got, side, src, affine in (("left", y[..., 0::2], left, lx, la), ("right", y[..., 1::2], right, rx, ra)):
        if affine:
            _close(got, side.fwd64(), TOL, f"shuffle_merge_fwd {mode} {name} {shape} h={h}")
        else:
            assert torch.equal(_bits(got), _bits(src)), f"{name}: the copy side is not a bit copy"


# --------------------------------------------------------------------------------------------- backward: reduce
@pytest.mark.parametrize("form", ["one_sided", "two_sided"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_merge_bwd_reduce(backend, shape, h, form):
    dev = backend
    n, hh, w = SHAPES[shape]
    M = n * hh * w
    g = _gen(200 * n * hh + h)
    right, left = _Side(g, SHAPES[shape], h, dev), _Side(g, SHAPES[shape], h, dev)
    dy = torch.randn(n, hh, w, 2 * h, generator=g)
    dyv, _ = _wide(dy, dev, off=4)
    two = form == "two_sided"
    sides = []
    for s, off in ((left, 4), (right, 0)):
        xv, _ = _wide(s.x, dev, off=off)
        sides.append((xv, s.dev_stats[0], s.dev_stats[1], s.dev_stats[2], "relu"))
    args = (sides[0] if two else None, sides[1])
    p0 = K.shuffle_merge_bwd_reduce(dyv, *args)
    p1 = K.shuffle_merge_bwd_reduce(dyv, *args)
    nblk = K.stats_blocks(M)
    assert tuple(p0.shape) == (4 if two else 2, nblk, h)
    assert torch.equal(p0.cpu(), p1.cpu()), "reduce partial rows differ between two calls"
    L, P = K.lib(), K.ptr
    for k, (s, half) in enumerate(((left, dy[..., 0::2]), (right, dy[..., 1::2])) if two else ((right, dy[..., 1::2]),)):
        _, dg64, db64, sg64, sgx64 = s.bwd64(half)
        what = f"shuffle_merge_bwd_reduce {form} side {k} {shape} h={h}"
        _close(p0[2 * k].double().sum(0), sg64, TOL, what + " sum g")
        _close(p0[2 * k + 1].double().sum(0), sgx64, TOL, what + " sum g*(x - mean)")
        # the plane pair, at the offset the header states, through the plain BatchNorm-backward finalize
        dgamma, dbeta, coef = torch.zeros(h, device=dev), torch.zeros(h, device=dev), torch.zeros(5, h, device=dev)
        ws, gamma = torch.zeros(L.sgx_reduce_workspace(nblk, h) // 4 + 1, device=dev), s.gamma.to(dev)
        rc = L.sgx_bn_bwd_finalize(P(p0) + 4 * (2 * k * nblk * h), nblk, M, h, P(gamma), P(s.dev_stats[2]), P(s.dev_stats[3]), P(dgamma), P(dbeta),
                                   P(coef), P(ws), ws.numel() * 4, None)
        assert rc == 0
        _close(dgamma, dg64, TOL_FIN, what + " dgamma")
        _close(dbeta, db64, TOL_FIN, what + " dbeta")


# --------------------------------------------------------------------------------------------- backward: apply
def _coef(parts, M, s, dev):
    h = parts.shape[2]
    return K._bn_bwd_coef(parts, M, s.gamma.to(dev), s.dev_stats[2], s.dev_stats[3], torch.zeros(h, device=dev), torch.zeros(h, device=dev), False)


@pytest.mark.parametrize("form", ["one_sided", "two_sided"])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_merge_bwd_apply(backend, shape, h, form):
    dev = backend
    n, hh, w = SHAPES[shape]
    M = n * hh * w
    g = _gen(300 * n * hh + h)
    right, left = _Side(g, SHAPES[shape], h, dev), _Side(g, SHAPES[shape], h, dev)
    dy = torch.randn(n, hh, w, 2 * h, generator=g)
    dyv, _ = _wide(dy, dev, off=4)
    two = form == "two_sided"
    halves = {"left": dy[..., 0::2], "right": dy[..., 1::2]}
    ref = {"left": left.bwd64(halves["left"])[0] if two else None, "right": right.bwd64(halves["right"])[0]}
    for in_place in (False, True):
        xl, _ = _wide(left.x, dev, off=4)
        xr, _ = _wide(right.x, dev)
        red = lambda s, xv: (xv, s.dev_stats[0], s.dev_stats[1], s.dev_stats[2], "relu")  # noqa: E731
        parts = K.shuffle_merge_bwd_reduce(dyv, red(left, xl) if two else None, red(right, xr))
        tl, tlbuf = (xl, None) if in_place else _wide(torch.zeros(n, hh, w, h), dev, off=4)
        tr, trbuf = (xr, None) if in_place else _wide(torch.zeros(n, hh, w, h), dev)
        if two:
            lspec = (xl, left.dev_stats[0], left.dev_stats[1], _coef(parts[:2], M, left, dev), "relu", tl)
        else:  # the copy side's target: the left channel slice of a wider gradient buffer, guards around it
            tl, tlbuf = _wide(torch.zeros(n, hh, w, h), dev, off=4)
            lspec = tl
        rspec = (xr, right.dev_stats[0], right.dev_stats[1], _coef(parts[2:] if two else parts, M, right, dev), "relu", tr)
        K.shuffle_merge_bwd_apply(dyv, lspec, rspec)
        tag = f"shuffle_merge_bwd_apply {form} {'in place' if in_place else 'out of place'} {shape} h={h}"
        _close(tr, ref["right"], TOL, tag + " dt right")
        if two:
            _close(tl, ref["left"], TOL, tag + " dt left")
        else:
            assert torch.equal(_bits(tl), _bits(halves["left"])), "the copy side's gradient is not dy[:, 0::2] bit for bit"
        for buf, off in ((tlbuf, 4), (trbuf, 0)):
            if buf is not None:
                assert _guards_ok(buf, off, h), "the apply sweep wrote outside a target slice"


@pytest.mark.parametrize("h", HS)
def test_merge_bwd_apply_identity_rows_pin_the_deinterleave(backend, h):
    """Identity coefficient rows (c1 = 1, the rest 0) and no activation: the apply sweep stores g itself - dt_right is dy[:, 1::2], dt_left
    dy[:, 0::2], bit for bit."""
    dev = backend
    n, hh, w = SHAPES["M70"]
    g = _gen(h)
    dy = torch.randn(n, hh, w, 2 * h, generator=g)
    x = torch.randn(n, hh, w, h, generator=g)
    one, zero = torch.ones(h, device=dev), torch.zeros(h, device=dev)
    coef = torch.zeros(5, h, device=dev)
    coef[0] = 1.0
    dyv, _ = _wide(dy, dev, off=4)
    tl, tr = torch.full((n, hh, w, h), GUARD, device=dev), torch.full((n, hh, w, h), GUARD, device=dev)
    K.shuffle_merge_bwd_apply(dyv, (x.to(dev), one, zero, coef, None, tl), (x.to(dev), one, zero, coef, None, tr))
    assert torch.equal(tl.cpu(), dy[..., 0::2]) and torch.equal(tr.cpu(), dy[..., 1::2])
    tl.fill_(GUARD), tr.fill_(GUARD)
    K.shuffle_merge_bwd_apply(dyv, tl, (x.to(dev), one, zero, coef, None, tr))
    assert torch.equal(tl.cpu(), dy[..., 0::2]) and torch.equal(tr.cpu(), dy[..., 1::2])


def test_mirrored_one_sided_forms(backend):
    """The modes are per side: the affine side on the LEFT and the copy on the right (no block of the network has it; the entry points do)."""
    dev = backend
    shape, h = SHAPES["M70"], 36
    n, hh, w = shape
    M = n * hh * w
    g = _gen(77)
    left = _Side(g, shape, h, dev)
    r = torch.randn(n, hh, w, h, generator=g)
    dy = torch.randn(n, hh, w, 2 * h, generator=g)
    lv, _ = _wide(left.x, dev, off=4)
    rv, _ = _wide(r, dev)
    dyv, _ = _wide(dy, dev, off=4)
    y = K.shuffle_merge(lv, rv, lscale=left.dev_stats[0], lshift=left.dev_stats[1], lact="relu").cpu()
    _close(y[..., 0::2], left.fwd64(), TOL, "shuffle_merge_fwd affine_copy left")
    assert torch.equal(_bits(y[..., 1::2]), _bits(r)), "right: the copy side is not a bit copy"
    dx64, dg64, db64, sg64, sgx64 = left.bwd64(dy[..., 0::2])
    parts = K.shuffle_merge_bwd_reduce(dyv, (lv, left.dev_stats[0], left.dev_stats[1], left.dev_stats[2], "relu"), None)
    assert tuple(parts.shape) == (2, K.stats_blocks(M), h)
    _close(parts[0].double().sum(0), sg64, TOL, "shuffle_merge_bwd_reduce left only sum g")
    _close(parts[1].double().sum(0), sgx64, TOL, "shuffle_merge_bwd_reduce left only sum g*(x - mean)")
    tl, tlbuf = _wide(torch.zeros(n, hh, w, h), dev, off=4)
    tr, trbuf = _wide(torch.zeros(n, hh, w, h), dev)
    K.shuffle_merge_bwd_apply(dyv, (lv, left.dev_stats[0], left.dev_stats[1], _coef(parts, M, left, dev), "relu", tl), tr)
    _close(tl, dx64, TOL, "shuffle_merge_bwd_apply left only dt left")
    assert torch.equal(_bits(tr), _bits(dy[..., 1::2])), "the copy side's gradient is not dy[:, 1::2] bit for bit"
    assert _guards_ok(tlbuf, 4, h) and _guards_ok(trbuf, 0, h)


# --------------------------------------------------------------------------------------------- refusals
BAD = ["h%4", "stride", "pointer", "null", "act-1", "act5", "M0"]


@pytest.mark.parametrize("which", BAD)
def test_refusals(backend, which):
    """Each entry point returns SGX_ERR_BAD_ARG and leaves every output at its guard value."""
    dev = backend
    M, h = 4, 8
    L, P = K.lib(), K.ptr
    a, b, dy = torch.ones(M, h, device=dev), torch.ones(M, h, device=dev), torch.ones(M, 2 * h, device=dev)
    vec = torch.ones(h, device=dev)
    coef = torch.zeros(5, h, device=dev)
    y = torch.full((M, 2 * h), GUARD, device=dev)
    parts = torch.full((4, 1, h), GUARD, device=dev)
    tl, tr = torch.full((M, h), GUARD, device=dev), torch.full((M, h), GUARD, device=dev)
    pa, ld, hh, mm, lact, ract, pb = P(a), h, h, M, 1, 1, P(b)
    if which == "h%4":
        hh = 6
    elif which == "stride":
        ld = h + 2
    elif which == "pointer":
        pa = P(a) + 8
    elif which == "null":
        pb = None
    elif which == "act-1":
        ract = -1
    elif which == "act5":
        lact = 5
    elif which == "M0":
        mm = 0
    v = P(vec)
    assert L.sgx_shuffle_merge_fwd(pa, ld, v, v, lact, pb, h, v, v, ract, P(y), 2 * h, mm, hh, None) == -1
    # (a NULL x makes a side of the reduce a copy, which is legal: there the NULL operand is the scale of an affine side)
    assert L.sgx_shuffle_merge_bwd_reduce(P(dy), 2 * h, pa, ld, v, v, v, lact, P(b), h, None if which == "null" else v, v, v, ract, mm, hh, P(parts), None) == -1
    assert L.sgx_shuffle_merge_bwd_apply(P(dy), 2 * h, pa, ld, v, v, P(coef), lact, P(tl), h, pb, h, v, v, P(coef), ract, P(tr), h, mm, hh, None) == -1
    if which == "null":  # also: a missing target, a missing gradient, no affine side at all
        assert L.sgx_shuffle_merge_fwd(P(a), h, v, v, 1, P(b), h, v, v, 1, None, 2 * h, M, h, None) == -1
        assert L.sgx_shuffle_merge_bwd_reduce(None, 2 * h, P(a), h, v, v, v, 1, P(b), h, v, v, v, 1, M, h, P(parts), None) == -1
        assert L.sgx_shuffle_merge_bwd_reduce(P(dy), 2 * h, None, 0, None, None, None, 0, None, 0, None, None, None, 0, M, h, P(parts), None) == -1
        assert L.sgx_shuffle_merge_bwd_apply(P(dy), 2 * h, None, 0, None, None, None, 0, None, h, P(b), h, v, v, P(coef), 1, P(tr), h, M, h, None) == -1
        assert L.sgx_shuffle_merge_bwd_apply(P(dy), 2 * h, None, 0, None, None, None, 0, P(tl), h, None, 0, None, None, None, 0, P(tr), h, M, h, None) == -1
    for name, t in (("y", y), ("partials", parts), ("d_left", tl), ("d_right", tr)):
        assert bool((t.cpu() == GUARD).all()), f"{which}: {name} was written by a refused call"
