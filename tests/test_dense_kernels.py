"""The DenseNet kernels of csrc/dense.h against plain torch in fp64 on the same fp32 operands:
  sgx_dense_stats_reduce / sgx_dense_bn_finalize   the block's shared statistics record and the BatchNorms finalised from its prefixes
  sgx_dense_bn_bwd_apply                           the BatchNorm backward that adds its input gradient to a channel prefix
  sgx_bn_act_avgpool2_fwd / _bwd_reduce / _bwd_apply   BatchNorm -> ReLU -> AvgPool2d(2, 2) as one sweep, forward and backward
Both back ends (the chip under -m gpu, the host emulation of the same sources otherwise) run the same cases.

Bars (relative, max-norm, against fp64; tests/test_dwconv_kernels.py, tests/test_bn_kernels.py): element outputs 2e-5, reduced quantities that
went through a finalize (scale, shift, mean, invstd, running statistics, dgamma, dbeta) 1e-4.  ReLU cases keep every fp64 pre-activation 1e-3
away from 0 (test_bn_kernels._away_from_kinks), so that a mask is never decided by rounding - except the case that pins the derivative AT 0.

One statement of the issue is mended here: it asks that at 7x5 the dx of the last row and column (outside every pooling window) be exactly 0
while dx matches fp64 autograd of a training-mode BatchNorm.  Both cannot hold: the BatchNorm's statistics include those pixels, so their
dx = c1 * (-mean g - xhat * mean(g * xhat)) is not zero.  What is exactly 0 there is g, the gradient that enters the BatchNorm backward; the test
pins it with identity coefficient rows (c1 = 1, everything else 0), under which the apply sweep stores g itself, and holds the true dx of
those pixels to the fp64 reference like every other pixel.
"""
import pytest
import torch
import torch.nn.functional as F

from util import rel_err

from super_gradients_amd import kernels as K
from super_gradients_amd._lib import SgxError
from test_bn_kernels import _away_from_kinks

TOL = 2e-5      # element outputs
TOL_FIN = 1e-4  # reduced quantities through a finalize
EPS, MOM = 1e-5, 0.1
GUARD = -7.25


def _close(got, ref, bar, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    e = rel_err(got, ref)
    print(f"DENSE_ERR {what} {bar:.3g} {e:.3e}")
    assert e <= bar, f"{what}: max err {e:.3e} of the tensor's max-abs > {bar:.3g}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _wide(t, device, extra=8, off=0, fill=GUARD):
    """NHWC tensor t as a channel slice [off, off + C) of a buffer `extra` channels wider, the rest holding `fill` -> (view, buffer)."""
    n, h, w, c = t.shape
    buf = torch.full((n, h, w, c + extra), fill, dtype=torch.float32, device=device)
    buf[..., off:off + c].copy_(t.to(device))
    return buf[..., off:off + c], buf


def _bn_affine(x, gamma, beta):
    """fp64 training-mode BatchNorm of an [..., C] tensor as (scale, shift, mean, invstd)."""
    xd = x.double().reshape(-1, x.shape[-1])
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    return scale, beta.double() - mean * scale, mean, invstd


def _nudged(x, gamma, beta):
    """x with no fp64 ReLU pre-activation of its training-mode BatchNorm within 1e-3 of 0."""
    shp = x.shape
    x2 = x.reshape(-1, shp[-1])

    def pre_of(t):
        s, b, _, _ = _bn_affine(t, gamma, beta)
        return t.double() * s + b

    def step_of():
        s, _, _, _ = _bn_affine(x2, gamma, beta)
        return 1.0 / s

    return _away_from_kinks(x2, pre_of, step_of, "relu").reshape(shp)


# --------------------------------------------------------------------------------------------- the statistics record
SLICES = (4, 32, 260)  # 260 channels: two 256-channel strips
C_TOTAL = sum(SLICES)
REC_LD = C_TOTAL + 8


@pytest.fixture
def record_case(backend):
    """A [2, 7, 5, C_TOTAL] concat buffer written slice by slice - the 32-channel slice by a 1x1 convolution whose epilogue leaves the
    partial rows, the others by plain copies with sgx_channel_stats_partial - and its record inside a wider one full of guard values."""
    dev = backend
    g = _gen(11)
    n, h, w = 2, 7, 5
    buf = torch.full((n, h, w, C_TOTAL), float("nan"), dtype=torch.float32, device=dev)
    rec = torch.full((2, REC_LD), GUARD, dtype=torch.float64, device=dev)
    off = 0
    for c in SLICES:
        view = buf[..., off:off + c]
        before = rec.clone()
        if c == 32:
            src = (torch.randn(n, h, w, 8, generator=g) * 1.5 + 0.3).to(dev)
            wt = K.to_ohwi((torch.randn(32, 8, 1, 1, generator=g) * 0.4).to(dev))
            _, parts = K.conv2d_fwd(src, wt, out=view, stat_partials=True)
        else:
            view.copy_((torch.randn(n, h, w, c, generator=g) * 2.0 + 0.5).to(dev))
            parts = K.channel_stats_partial(view)
        assert K.dense_stats_reduce(parts, rec, off) == 1
        keep = torch.ones(REC_LD, dtype=torch.bool)
        keep[off:off + c] = False
        assert torch.equal(rec.cpu()[:, keep], before.cpu()[:, keep]), f"slice {c}: record entries outside the slice changed"
        off += c
    return dev, buf, rec, n * h * w


def test_record_sums(record_case):
    dev, buf, rec, M = record_case
    xd = buf.cpu().double().reshape(M, C_TOTAL)
    _close(rec[0, :C_TOTAL], xd.sum(0), TOL, "stats_reduce sum")
    _close(rec[1, :C_TOTAL], (xd * xd).sum(0), TOL, "stats_reduce sum of squares")
    assert bool((rec.cpu()[:, C_TOTAL:] == GUARD).all())


@pytest.mark.parametrize("c_in", [20, 36, C_TOTAL], ids=["inside_slice", "slice_boundary", "c_total"])
def test_record_finalize(record_case, c_in):
    dev, buf, rec, M = record_case
    g = _gen(c_in)
    gamma, beta = torch.rand(c_in, generator=g) + 0.5, torch.randn(c_in, generator=g) * 0.3
    rm0, rv0 = torch.randn(c_in, generator=g) * 0.2, torch.rand(c_in, generator=g) + 0.5
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    before = rec.clone()
    scale, shift, mean, invstd = K.dense_bn_finalize(rec, M, c_in, gamma.to(dev), beta.to(dev), EPS, MOM, rm, rv)
    assert torch.equal(rec.cpu(), before.cpu()), "the finalize wrote the record"
    x = buf.cpu()[..., :c_in]
    s64, t64, m64, i64 = _bn_affine(x, gamma, beta)
    for name, got, ref in (("scale", scale, s64), ("shift", shift, t64), ("save_mean", mean, m64), ("save_invstd", invstd, i64)):
        _close(got, ref, TOL_FIN, f"dense_bn_finalize[{c_in}] {name}")
    rm64, rv64 = rm0.double(), rv0.double()
    F.batch_norm(x.double().permute(0, 3, 1, 2), rm64, rv64, gamma.double(), beta.double(), True, MOM, EPS)
    _close(rm, rm64, TOL_FIN, f"dense_bn_finalize[{c_in}] running_mean")
    _close(rv, rv64, TOL_FIN, f"dense_bn_finalize[{c_in}] running_var")


# --------------------------------------------------------------------------------------------- the accumulating BatchNorm backward
@pytest.mark.parametrize("act", ["relu", None], ids=["relu", "none"])
@pytest.mark.parametrize("c_in", [4, 36, 260])
@pytest.mark.parametrize("shape", [(1, 6, 3), (2, 7, 5), (4, 16, 16)], ids=["M18", "M70", "M1024"])
def test_accumulating_apply(backend, shape, c_in, act):
    dev = backend
    n, h, w = shape
    g = _gen(1000 * n * h + c_in)
    gamma, beta = torch.rand(c_in, generator=g) + 0.5, torch.randn(c_in, generator=g) * 0.3
    x = torch.randn(n, h, w, c_in, generator=g) * 2.0 + 0.5
    if act == "relu":
        x = _nudged(x, gamma, beta)
    dy = torch.randn(n, h, w, c_in, generator=g)
    prior = torch.randn(n, h, w, c_in + 8, generator=g)
    # fp64 reference
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.batch_norm(xd.permute(0, 3, 1, 2), None, None, wd, bd, True, MOM, EPS)
    (F.relu(y) if act == "relu" else y).backward(dy.double().permute(0, 3, 1, 2))
    # kernels: statistics -> finalize -> reduce -> finalize -> dx += ...
    xv, _ = _wide(x, dev)  # (a channel prefix of a wider buffer, as in the block)
    M = n * h * w
    scale, shift, mean, invstd = K.bn_finalize(K.channel_stats_partial(xv), M, gamma.to(dev), beta.to(dev), EPS, MOM, None, None)
    outs = []
    for _ in range(2):
        gbuf = prior.clone().to(dev)
        dgamma, dbeta = torch.zeros(c_in, device=dev), torch.zeros(c_in, device=dev)
        K.dense_bn_bwd(dy.to(dev), xv, scale, shift, gamma.to(dev), mean, invstd, dgamma, dbeta, gbuf[..., :c_in], act=act)
        outs.append(gbuf.cpu())
    got = outs[0]
    assert torch.equal(got[..., c_in:], prior[..., c_in:]), "channels behind the prefix changed"
    assert torch.equal(outs[0], outs[1]), "a second call from the same inputs differs"
    _close(got[..., :c_in], prior[..., :c_in].double() + xd.grad, TOL, "dense_bn_bwd_apply prior + dx")
    _close(got[..., :c_in].double() - prior[..., :c_in].double(), xd.grad, TOL_FIN, "dense_bn_bwd_apply dx")
    _close(dgamma, wd.grad, TOL_FIN, "dense_bn_bwd dgamma")
    _close(dbeta, bd.grad, TOL_FIN, "dense_bn_bwd dbeta")


# --------------------------------------------------------------------------------------------- BatchNorm -> ReLU -> 2x2 average pool
@pytest.mark.parametrize("shape", [(2, 4, 4, 8), (2, 7, 5, 36), (1, 2, 2, 260)], ids=["2x4x4x8", "2x7x5x36", "1x2x2x260"])
def test_fused_pool_sweeps(backend, shape):
    dev = backend
    n, h, w, c = shape
    g = _gen(h * 100 + c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    x = _nudged(torch.randn(n, h, w, c, generator=g) * 2.0 + 0.5, gamma, beta)
    dz = torch.randn(n, h // 2, w // 2, c, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    z64 = F.avg_pool2d(F.relu(F.batch_norm(xd.permute(0, 3, 1, 2), None, None, wd, bd, True, MOM, EPS)), 2)
    z64.backward(dz.double().permute(0, 3, 1, 2))

    xv, _ = _wide(x, dev)                                 # input: a prefix view of a wider buffer
    zv, zbuf = _wide(torch.zeros(n, h // 2, w // 2, c), dev, off=4)  # output: a slice view
    dxv, dxbuf = _wide(torch.zeros(n, h, w, c), dev)
    dzv, _ = _wide(dz, dev, off=4)
    M = n * h * w
    scale, shift, mean, invstd = K.bn_finalize(K.channel_stats_partial(xv), M, gamma.to(dev), beta.to(dev), EPS, MOM, None, None)
    K.bn_act_avgpool2_fwd(xv, scale, shift, act="relu", out=zv)
    _close(zv, z64.detach().permute(0, 2, 3, 1), TOL, f"bn_act_avgpool2_fwd {shape}")
    assert bool((zbuf.cpu()[..., :4] == GUARD).all()) and bool((zbuf.cpu()[..., 4 + c:] == GUARD).all()), "forward wrote outside its slice"

    p0 = K.bn_act_avgpool2_bwd_reduce(dzv, xv, scale, shift, mean, act="relu")
    p1 = K.bn_act_avgpool2_bwd_reduce(dzv, xv, scale, shift, mean, act="relu")
    assert tuple(p0.shape) == (2, K.stats_blocks(M), c)
    assert torch.equal(p0.cpu(), p1.cpu()), "reduce partial rows differ between two calls"
    dgamma, dbeta = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    K.bn_act_avgpool2_bwd(dzv, xv, scale, shift, gamma.to(dev), mean, invstd, dgamma, dbeta, dxv, act="relu")
    _close(dxv, xd.grad, TOL, f"bn_act_avgpool2_bwd dx {shape}")
    _close(dgamma, wd.grad, TOL_FIN, f"bn_act_avgpool2_bwd dgamma {shape}")
    _close(dbeta, bd.grad, TOL_FIN, f"bn_act_avgpool2_bwd dbeta {shape}")
    assert bool((dxbuf.cpu()[..., c:] == GUARD).all()), "backward wrote behind its prefix"


def test_fused_pool_zero_preactivation_and_unused_border(backend):
    """scale 1, shift 0 and exact zeros in x: the derivative at a pre-activation of exactly 0 is 0.  With identity coefficient rows the apply
    sweep stores g itself: a quarter of the window's dz where x > 0, and exactly 0 on the last row and column of the 7x5 map."""
    dev = backend
    n, h, w, c = 2, 7, 5, 36
    g = _gen(5)
    x = torch.randn(n, h, w, c, generator=g)
    x[torch.rand(n, h, w, c, generator=g) < 0.3] = 0.0
    dz = torch.randn(n, 3, 2, c, generator=g)
    one, zero = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    z = K.bn_act_avgpool2_fwd(x.to(dev), one, zero, act="relu")
    _close(z, F.avg_pool2d(F.relu(x.double().permute(0, 3, 1, 2)), 2).permute(0, 2, 3, 1), TOL, "bn_act_avgpool2_fwd identity")
    coef = torch.zeros(5, c, device=dev)
    coef[0] = 1.0
    dx = torch.full((n, h, w, c), float("nan"), device=dev)
    K.bn_act_avgpool2_bwd_apply(dz.to(dev), x.to(dev), one, zero, coef, dx, act="relu")
    up = torch.zeros(n, h, w, c)
    up[:, :6, :4] = (0.25 * dz).repeat_interleave(2, 1).repeat_interleave(2, 2)
    want = torch.where(x > 0, up, torch.zeros(()))
    dx = dx.cpu()
    assert torch.equal(dx, want), "g != dz / 4 * 1[x > 0]"
    assert bool((dx[:, 6] == 0).all()) and bool((dx[:, :, 4] == 0).all()), "the row / column outside every window received gradient"
    assert bool((dx[x == 0] == 0).all()), "derivative at a pre-activation of exactly 0 is not 0"
    parts = K.bn_act_avgpool2_bwd_reduce(dz.to(dev), x.to(dev), one, zero, zero, act="relu")
    _close(parts[0].sum(0), want.double().reshape(-1, c).sum(0), TOL_FIN, "bn_act_avgpool2_bwd_reduce sum g")
    _close(parts[1].sum(0), (want.double() * x.double()).reshape(-1, c).sum(0), TOL_FIN, "bn_act_avgpool2_bwd_reduce sum g*x")


# --------------------------------------------------------------------------------------------- rejections
def _bad_views(dev, n, h, w, c):
    """(name, x-like view) whose channel count, address or row stride breaks the 16-byte rules; c is a valid channel count."""
    m = n * h * w
    flat = torch.zeros(m * (c + 2) + 8, device=dev)
    return [("C % 4 != 0", torch.zeros(n, h, w, c + 2, device=dev)),
            ("misaligned pointer", flat[1:1 + m * c].view(n, h, w, c)),
            ("row stride % 4 != 0", flat[: m * (c + 2)].view(n, h, w, c + 2)[..., :c])]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["channels", "pointer", "stride"])
def test_rejections(backend, which):
    dev = backend
    n, h, w, c = 1, 2, 2, 8
    name, bad = _bad_views(dev, n, h, w, c)[which]
    cb = bad.shape[3]
    good = torch.zeros(n, h, w, cb, device=dev)
    vec = torch.ones(max(cb, 8), device=dev)[:cb]
    coef = torch.zeros(5, cb, device=dev)
    out = torch.full((n, h, w, cb), GUARD, device=dev)
    zout = torch.full((n, 1, 1, cb), GUARD, device=dev)
    dzg = torch.zeros(n, 1, 1, cb, device=dev)
    calls = {
        "dense_bn_bwd_apply": lambda: K.dense_bn_bwd_apply(good, bad, vec, vec, coef, out),
        "bn_act_avgpool2_fwd": lambda: K.bn_act_avgpool2_fwd(bad, vec, vec, act="relu", out=zout),
        "bn_act_avgpool2_bwd_reduce": lambda: K.bn_act_avgpool2_bwd_reduce(dzg, bad, vec, vec, vec, act="relu"),
        "bn_act_avgpool2_bwd_apply": lambda: K.bn_act_avgpool2_bwd_apply(dzg, bad, vec, vec, coef, out, act="relu"),
    }
    for kname, call in calls.items():
        with pytest.raises(SgxError, match="status -1"):
            call()
        assert bool((out.cpu() == GUARD).all()) and bool((zout.cpu() == GUARD).all()), f"{kname} ({name}): something was written"
    # the record entries: slice width / offset / record stride / address
    rec = torch.full((2, 16), GUARD, dtype=torch.float64, device=dev)
    flat = torch.zeros(2 * 1 * 8 + 8, device=dev)
    parts_ok = flat[:16].view(2, 1, 8)
    st = [torch.full((8,), GUARD, device=dev) for _ in range(2)]
    L, P = K.lib(), K.ptr
    bad_calls = {
        0: [lambda: L.sgx_dense_stats_reduce(P(parts_ok), 1, 6, P(rec), 16, 0, None, 0, None),
            lambda: L.sgx_dense_bn_finalize(P(rec), 16, 4, 6, None, None, EPS, MOM, None, None, None, None, P(st[0]), P(st[1]), None)],
        1: [lambda: L.sgx_dense_stats_reduce(P(flat[1:17]), 1, 8, P(rec), 16, 0, None, 0, None),
            lambda: L.sgx_dense_bn_finalize(P(rec.flatten()[1:]), 16, 4, 8, None, None, EPS, MOM, None, None, None, None, P(st[0]), P(st[1]), None)],
        2: [lambda: L.sgx_dense_stats_reduce(P(parts_ok), 1, 8, P(rec), 14, 0, None, 0, None),
            lambda: L.sgx_dense_stats_reduce(P(parts_ok), 1, 8, P(rec), 16, 2, None, 0, None),
            lambda: L.sgx_dense_bn_finalize(P(rec), 14, 4, 8, None, None, EPS, MOM, None, None, None, None, P(st[0]), P(st[1]), None)],
    }[which]
    for call in bad_calls:
        assert call() == -1
    assert bool((rec.cpu() == GUARD).all()) and all(bool((t.cpu() == GUARD).all()) for t in st), f"record entry points ({name}): something was written"
