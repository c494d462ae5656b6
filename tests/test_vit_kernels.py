"""The Vision Transformer's glue kernels (csrc/vit.h: sgx_attn_fwd / _bwd, sgx_layernorm_fwd / _bwd, sgx_gelu_fwd / _bwd, sgx_patch_rows,
sgx_token_assemble_fwd / _bwd) against torch in fp64 on the CPU, on the chip and on the host emulation of the same sources.

Bars (the project's own, tests/test_se_kernels.py): 2e-5 of the tensor's max-abs for element-wise results, 1e-4 for results that are sums over
rows (dgamma, dbeta, dpos, dcls).  Every case runs with contiguous operands and with every operand a channel slice of a wider NaN-filled
buffer (a different pad and offset per operand, all multiples of 4 floats): the surroundings of every output keep their bits, no output element
is NaN.  Every comparison prints `VIT_ERR <kernel> <quantity> <bar> <measured>` before it asserts (pytest -rP shows the lines).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from util import rel_err

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5
TOL_SUM = 1e-4
NAN = float("nan")
LAYOUTS = ["slices", "contiguous"]
# (extra floats per token, channel offset) of operand k as a channel slice of a wider NaN-filled buffer
SLICE = [(8, 4), (16, 8), (12, 0), (24, 12), (20, 4), (28, 0), (36, 16), (32, 8)]


def _seed(*parts):
    return sum((i + 1) * 7919 * (sum(map(ord, p)) if isinstance(p, str) else int(p)) for i, p in enumerate(parts)) % (2 ** 31)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _view(shape, dev, layout, k, fill=None):
    """A [B, T, 1, C] view (NaN-filled, or holding `fill`): contiguous, or a channel slice of a wider NaN buffer."""
    b, t, one, c = shape
    pad, off = (0, 0) if layout == "contiguous" else SLICE[k]
    buf = torch.full((b, t, 1, c + pad), NAN, dtype=torch.float32, device=dev)
    v = buf[..., off:off + c]
    if fill is not None:
        v.copy_(fill.reshape(shape).to(dev))
    return v


def _base(v):
    return v if v._base is None else v._base


def _surround(v):
    """The bits of v's base buffer with v's own channels blanked: equal before and after a call that may only write v."""
    base = _base(v)
    b = base.clone()
    lo = (v.storage_offset() - base.storage_offset()) % base.shape[-1]
    b[..., lo:lo + v.shape[-1]] = 0
    return _bits(b)


def _close(got, ref, tol, kernel, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"{kernel} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    e = rel_err(got, ref)
    print(f"VIT_ERR {kernel} {what} {tol:g} {e:.3e}")
    assert e <= tol, f"{kernel} {what}: max err {e:.3e} of the tensor's max-abs > {tol}"


class _Watch:
    """Outputs of one call: their surroundings before it, checked after it."""

    def __init__(self, *outs):
        self.outs = outs
        self.before = [_surround(o) for o in outs]

    def check(self, what):
        for i, (o, b) in enumerate(zip(self.outs, self.before)):
            assert torch.equal(_surround(o), b), f"{what}: output {i} wrote outside its view"
            assert not bool(torch.isnan(o).any()), f"{what}: output {i} has NaN elements"


# --------------------------------------------------------------------------------------------- attention
ATTN_FIXED = [(2, 3, 197, 64, 1.0), (2, 3, 197, 64, 4.0), (2, 4, 64, 16, 6.0), (2, 1, 65, 80, 2.0), (1, 2, 1, 16, 1.0)]


@functools.lru_cache(maxsize=None)
def _attn_case(B, H, T, d, mag):
    """Inputs and the fp64 autograd reference, built once and shared by both back ends and both layouts."""
    g = torch.Generator().manual_seed(_seed(B, H, T, d, int(mag * 10)))
    D = H * d
    qkv = torch.randn(B, T, 3 * D, generator=g)
    qkv[..., :2 * D] *= mag
    do = torch.randn(B, T, D, generator=g)
    scale = d ** -0.5
    q, k, v = [t.double().reshape(B, T, H, d).permute(0, 2, 1, 3).clone().requires_grad_(True) for t in qkv.split(D, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * scale
    o = s.softmax(-1) @ v
    o.backward(do.double().reshape(B, T, H, d).permute(0, 2, 1, 3))
    back = lambda t: t.detach().permute(0, 2, 1, 3).reshape(B, T, 1, D)  # noqa: E731
    return dict(qkv=qkv, do=do, scale=scale, o=back(o), lse=torch.logsumexp(s.detach(), -1), dq=back(q.grad), dk=back(k.grad), dv=back(v.grad),
                max_logit=float(s.detach().abs().max()))


def _attn_run(case, B, H, T, d, dev, layout):
    D = H * d
    qkv = _view((B, T, 1, 3 * D), dev, layout, 0, case["qkv"])
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    o = _view((B, T, 1, D), dev, layout, 1)
    w = _Watch(o)
    _, lse = K.attn_fwd(q, k, v, H, case["scale"], out=o)
    w.check("attn_fwd")
    do = _view((B, T, 1, D), dev, layout, 1, case["do"])  # (dO shares o's strides: the same pad)
    dqkv = _view((B, T, 1, 3 * D), dev, layout, 3)
    w = _Watch(dqkv)
    K.attn_bwd(q, k, v, o, do, lse, H, case["scale"], dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:])
    w.check("attn_bwd")
    return qkv, o, lse, do, dqkv


def _attn_check(B, H, T, d, mag, dev, layout):
    case = _attn_case(B, H, T, d, mag)
    D = H * d
    qkv, o, lse, do, dqkv = _attn_run(case, B, H, T, d, dev, layout)
    tag = f"attn[{B},{H},{T},{d},x{mag:g},{layout}]"
    _close(o, case["o"], TOL, tag, "o")
    _close(lse, case["lse"], TOL, tag, "lse")
    for i, name in enumerate(("dq", "dk", "dv")):
        _close(dqkv[..., i * D:(i + 1) * D], case[name], TOL, tag, name)
    # twice: the same bits
    again = _view((B, T, 1, 3 * D), dev, layout, 3)
    K.attn_bwd(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], o, do, lse, H, case["scale"], again[..., :D], again[..., D:2 * D], again[..., 2 * D:])
    assert torch.equal(_bits(again), _bits(dqkv)), f"{tag}: the backward does not repeat its bits"
    # head h of the multi-head call == a one-head call on that head's slices, bit for bit
    if H > 1:
        for h in range(H):
            sl = lambda t, part=0: t[..., part * D + h * d: part * D + (h + 1) * d]  # noqa: E731
            o1, lse1 = K.attn_fwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), 1, case["scale"])
            assert torch.equal(_bits(o1), _bits(sl(o))) and torch.equal(_bits(lse1[:, 0]), _bits(lse[:, h])), f"{tag}: head {h} forward differs from the one-head call"
            g1 = torch.full((B, T, 1, 3 * d), NAN, device=dev)
            K.attn_bwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), sl(o), sl(do), lse[:, h:h + 1].contiguous(), 1, case["scale"], g1[..., :d], g1[..., d:2 * d], g1[..., 2 * d:])
            for part in range(3):
                assert torch.equal(_bits(g1[..., part * d:(part + 1) * d]), _bits(sl(dqkv, part))), f"{tag}: head {h} backward part {part} differs from the one-head call"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ATTN_FIXED[:4], ids=lambda s: "x".join(f"{v:g}" for v in s))
def test_attention(backend, shape, layout):
    B, H, T, d, mag = shape
    case = _attn_case(*shape)
    print(f"VIT_ERR attn[{shape}] max|logit| - {case['max_logit']:.1f}")
    if shape == ATTN_FIXED[1]:
        assert case["max_logit"] > 60, "the case must overflow a softmax that does not subtract the row maximum"
    if shape == ATTN_FIXED[2]:
        assert case["max_logit"] > 120
    _attn_check(B, H, T, d, mag, backend, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_attention_one_token(backend, layout):
    """T = 1: the softmax is 1, o = v, dv = dO, and dq = dk = 0 - compared absolutely: ds is the rounding of two d-term dot products of
    dO and v, so |dq| <= bar * scale * max_row(sum |dO| |v|) * max |k| (the size dq would have if ds were of order one)."""
    B, H, T, d, mag = ATTN_FIXED[4]
    case = _attn_case(B, H, T, d, mag)
    D = H * d
    qkv, o, lse, do, dqkv = _attn_run(case, B, H, T, d, backend, layout)
    assert torch.equal(_bits(o), _bits(qkv[..., 2 * D:])), "one token: o must equal v"
    assert torch.equal(_bits(dqkv[..., 2 * D:]), _bits(do)), "one token: dv must equal dO"
    _close(lse, case["lse"], TOL, "attn[one token]", "lse")
    size = case["scale"] * float((case["do"].abs() * case["qkv"][..., 2 * D:].abs()).reshape(B, T, H, d).sum(-1).max())
    for i, (name, other) in enumerate((("dq", 1), ("dk", 0))):
        bound = TOL * size * float(case["qkv"][..., other * D:(other + 1) * D].abs().max())
        e = float(dqkv[..., i * D:(i + 1) * D].abs().max())
        print(f"VIT_ERR attn[one token,{layout}] {name} {bound:.3e} {e:.3e}")
        assert e <= bound, f"one token: |{name}| = {e:.3e} > {bound:.3e}"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_attention_around_the_tiles(backend, delta, layout):
    """T one below, at and one above the own-row tile, the staged tile and the matrix-instruction tile of the kernels (the first two from
    the library's own geometry query)."""
    tq, tk = K.lib().sgx_attn_tile_rows(0), K.lib().sgx_attn_tile_rows(1)
    assert (tq, tk) == (64, 32), "ATT_TQ / ATT_TK changed: DESIGN.md 19 and the shapes here follow them"
    for t in sorted({tq, tk, 16}):  # (16: the rows of one matrix-instruction tile, the step inside a staged tile)
        _attn_check(2, 2, t + delta, 16, 1.0, backend, layout)


# --------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(394, 768), (5, 1280), (130, 64), (33, 4)]
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _ln_case(M, C):
    g = torch.Generator().manual_seed(_seed(M, C))
    x = 2.0 * torch.randn(M, C, generator=g) + 0.7  # a non-zero mean: a one-pass variance shows
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dy, addend = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xd, (C,), gd, bd, EPS)
    y.backward(dy.double())
    mean = x.double().mean(-1)
    rstd = (x.double().var(-1, unbiased=False) + EPS).rsqrt()
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, addend=addend, dg0=dg0, db0=db0, y=y.detach(), mean=mean, rstd=rstd, dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)


def _ln_check(M, C, dev, layout):
    case = _ln_case(M, C)
    rows_per = K.lib().sgx_layernorm_bwd_block_rows()
    assert K.lib().sgx_layernorm_bwd_workspace(M, C) == 2 * (-(-M // rows_per)) * C * 4 + 256
    shape = (1, M, 1, C)
    tag = f"layernorm[{M},{C},{layout}]"
    x = _view(shape, dev, layout, 0, case["x"])
    gamma, beta = case["gamma"].to(dev), case["beta"].to(dev)
    y = _view(shape, dev, layout, 1)
    w = _Watch(y)
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, EPS, out=y)
    w.check(tag)
    _close(y, case["y"].reshape(shape), TOL, tag, "y")
    _close(mean, case["mean"], TOL, tag, "mean")
    _close(rstd, case["rstd"], TOL, tag, "rstd")
    dy = _view(shape, dev, layout, 2, case["dy"])
    addend = _view(shape, dev, layout, 3, case["addend"])
    results = []
    for rep in range(2):
        dgamma, dbeta = case["dg0"].clone().to(dev), case["db0"].clone().to(dev)
        dx, dxa = _view(shape, dev, layout, 4), _view(shape, dev, layout, 5)
        w = _Watch(dx, dxa)
        K.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, out=dx)
        K.layernorm_bwd(dy, x, gamma, mean, rstd, addend=addend, out=dxa)  # (no parameter gradients: dgamma / dbeta stay)
        w.check(tag)
        results.append((dx, dxa, dgamma, dbeta))
    dx, dxa, dgamma, dbeta = results[0]
    _close(dx, case["dx"].reshape(shape), TOL, tag, "dx")
    _close(dxa, (case["dx"] + case["addend"].double()).reshape(shape), TOL, tag, "dx+addend")
    _close(dgamma.cpu().double() - case["dg0"].double(), case["dgamma"], TOL_SUM, tag, "dgamma (added onto the arena view)")
    _close(dbeta.cpu().double() - case["db0"].double(), case["dbeta"], TOL_SUM, tag, "dbeta (added onto the arena view)")
    for a, b in zip(results[0], results[1]):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: the backward does not repeat its bits"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm(backend, shape, layout):
    _ln_check(*shape, backend, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_layernorm_around_the_row_block(backend, delta, layout):
    rows_per = K.lib().sgx_layernorm_bwd_block_rows()
    assert rows_per == 64, "LN_BWD_BLOCK_ROWS changed: DESIGN.md 19 follows it"
    _ln_check(rows_per + delta, 24, backend, layout)


def test_layernorm_class_token_rows(backend):
    """The head's form: a [B, 1, 1, D] view of a [B, T, 1, D] stream (image stride T * D) in, a view of the same kind out."""
    B, T, D = 3, 5, 24
    case = _ln_case(B, D)
    stream = torch.full((B, T, 1, D), NAN, device=backend)
    stream[:, :1].copy_(case["x"].reshape(B, 1, 1, D))
    gamma, beta = case["gamma"].to(backend), case["beta"].to(backend)
    y, mean, rstd = K.layernorm_fwd(stream[:, :1], gamma, beta, EPS)
    _close(y, case["y"].reshape(B, 1, 1, D), TOL, "layernorm[class rows]", "y")
    dfull = torch.zeros(B, T, 1, D, device=backend)
    dgamma, dbeta = torch.zeros(D, device=backend), torch.zeros(D, device=backend)
    K.layernorm_bwd(case["dy"].reshape(B, 1, 1, D).to(backend), stream[:, :1], gamma, mean, rstd, dgamma, dbeta, out=dfull[:, :1])
    _close(dfull[:, :1], case["dx"].reshape(B, 1, 1, D), TOL, "layernorm[class rows]", "dx")
    assert not bool(dfull[:, 1:].any()), "rows other than the class token's were written"
    _close(dgamma, case["dgamma"], TOL_SUM, "layernorm[class rows]", "dgamma")


# --------------------------------------------------------------------------------------------- GELU
@functools.lru_cache(maxsize=None)
def _gelu_case(shape):
    g = torch.Generator().manual_seed(_seed(*shape))
    x = torch.rand(shape, generator=g) * 12.0 - 6.0
    x.view(-1)[:5] = torch.tensor([0.0, 1e-4, -1e-4, 6.0, -6.0])
    dy = torch.randn(shape, generator=g)
    xd = x.double().requires_grad_(True)
    y = F.gelu(xd)
    y.backward(dy.double())
    return dict(x=x, dy=dy, y=y.detach(), dx=xd.grad)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 7, 1, 12), (2, 197, 1, 3072)], ids=["2x7x12", "2x197x3072"])
def test_gelu(backend, shape, layout):
    case = _gelu_case(shape)
    tag = f"gelu[{shape},{layout}]"
    x, dy = _view(shape, backend, layout, 0, case["x"]), _view(shape, backend, layout, 1, case["dy"])
    y, dx = _view(shape, backend, layout, 2), _view(shape, backend, layout, 3)
    w = _Watch(y, dx)
    K.gelu_fwd(x, out=y)
    K.gelu_bwd(dy, x, out=dx)
    w.check(tag)
    _close(y, case["y"], TOL, tag, "y")
    _close(dx, case["dx"], TOL, tag, "dx")
    inplace = dy.clone() if layout == "contiguous" else _view(shape, backend, layout, 1, case["dy"])
    K.gelu_bwd(inplace, x, out=inplace)
    assert torch.equal(_bits(inplace), _bits(dx)), f"{tag}: the in-place backward differs"


# --------------------------------------------------------------------------------------------- patch rows, token assembly
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", [(2, 32, 32, 8, 8), (3, 48, 80, 16, 16)], ids=["32x32p8", "48x80p16"])
def test_patch_rows_bit_exact(backend, geom, layout):
    B, H, W, ph, pw = geom
    C = 4
    gh, gw = H // ph, W // pw
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(_seed(*geom)))
    want = x.view(B, gh, ph, gw, pw, C).permute(0, 1, 3, 2, 4, 5).reshape(B, gh * gw, 1, ph * pw * C)  # unfold-style indexing, (py, px, c) order
    pad, off = (0, 0) if layout == "contiguous" else SLICE[0]
    buf = torch.full((B, H, W, C + pad), NAN, device=backend)
    xv = buf[..., off:off + C]
    xv.copy_(x.to(backend))
    out = _view((B, gh * gw, 1, ph * pw * C), backend, layout, 1)
    w = _Watch(out)
    K.patch_rows(xv, ph, pw, out=out)
    w.check("patch_rows")
    assert torch.equal(_bits(out), _bits(want)), "patch rows differ from unfold-style indexing"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [2, 17])
def test_token_assembly(backend, B, T, layout):
    D = 12
    g = torch.Generator().manual_seed(_seed(B, T))
    patch, cls, pos = torch.randn(B, T - 1, D, generator=g), torch.randn(1, 1, D, generator=g), torch.randn(1, T, D, generator=g)
    want = torch.cat((cls.expand(B, 1, D), patch), dim=1) + pos
    pv = _view((B, T - 1, 1, D), backend, layout, 0, patch)
    out = _view((B, T, 1, D), backend, layout, 1)
    w = _Watch(out)
    K.token_assemble_fwd(pv, cls.to(backend), pos.to(backend), out=out)
    w.check("token_assemble_fwd")
    assert torch.equal(_bits(out), _bits(want.reshape(B, T, 1, D))), "token assembly differs from cat + add"
    dx = torch.randn(B, T, D, generator=g)
    dcls0, dpos0 = torch.randn(1, 1, D, generator=g), torch.randn(1, T, D, generator=g)
    dcls, dpos = dcls0.clone().to(backend), dpos0.clone().to(backend)
    K.token_assemble_bwd(_view((B, T, 1, D), backend, layout, 2, dx), dcls, dpos)
    ref = dx.double().sum(0, keepdim=True)
    tag = f"token_assemble_bwd[{B},{T},{layout}]"
    _close(dpos.cpu().double() - dpos0.double(), ref, TOL_SUM, tag, "dpos (added)")
    _close(dcls.cpu().double() - dcls0.double(), ref[:, :1], TOL_SUM, tag, "dcls (added)")


# --------------------------------------------------------------------------------------------- refusals
def _refused(call, *outs):
    before = [_bits(_base(o)) for o in outs]
    with pytest.raises(_lib.SgxError):
        call()
    for o, b in zip(outs, before):
        assert torch.equal(_bits(_base(o)), b), "a refused call wrote its output"


def test_argument_refusals(backend):
    dev = backend
    full = lambda *s: torch.full(s, NAN, device=dev)  # noqa: E731
    # head width not a multiple of 4
    qkv, o = torch.zeros(1, 3, 1, 18, device=dev), full(1, 3, 1, 6)
    _refused(lambda: K.attn_fwd(qkv[..., :6], qkv[..., 6:12], qkv[..., 12:], 1, 1.0, out=o), o)
    # a pixel stride that is not a multiple of 4
    qkv, o = torch.zeros(1, 3, 1, 26, device=dev), full(1, 3, 1, 8)
    _refused(lambda: K.attn_fwd(qkv[..., :8], qkv[..., 8:16], qkv[..., 16:24], 1, 1.0, out=o), o)
    x, y = torch.zeros(1, 3, 1, 10, device=dev), full(1, 3, 1, 8)
    _refused(lambda: K.gelu_fwd(x[..., :8], out=y), y)
    _refused(lambda: K.layernorm_fwd(x[..., :8], torch.ones(8, device=dev), torch.zeros(8, device=dev), EPS, out=y), y)
    # a misaligned pointer (one float into a buffer whose strides are fine)
    x = torch.zeros(1, 3, 1, 12, device=dev)
    _refused(lambda: K.gelu_fwd(x[..., 1:9], out=y), y)
    _refused(lambda: K.layernorm_fwd(x[..., 1:9], torch.ones(8, device=dev), torch.zeros(8, device=dev), EPS, out=y), y)
    qkv, o = torch.zeros(1, 3, 1, 28, device=dev), full(1, 3, 1, 8)
    _refused(lambda: K.attn_fwd(qkv[..., 1:9], qkv[..., 9:17], qkv[..., 17:25], 1, 1.0, out=o), o)
    yo = full(1, 3, 1, 12)
    _refused(lambda: K.token_assemble_fwd(torch.zeros(1, 2, 1, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(3, 8, device=dev), out=yo[..., 1:9]), yo)
    # a channel count that is not a multiple of 4
    x6, y6 = torch.zeros(1, 3, 1, 6, device=dev), full(1, 3, 1, 6)
    _refused(lambda: K.layernorm_fwd(x6, torch.ones(6, device=dev), torch.zeros(6, device=dev), EPS, out=y6), y6)
    _refused(lambda: K.gelu_fwd(x6, out=y6), y6)
    dx6 = full(1, 3, 1, 6)
    _refused(lambda: K.layernorm_bwd(x6, x6, torch.ones(6, device=dev), torch.zeros(3, device=dev), torch.ones(3, device=dev), out=dx6), dx6)
    rows = full(1, 4, 1, 6 * 4)
    _refused(lambda: K.patch_rows(torch.zeros(1, 4, 4, 6, device=dev), 2, 2, out=rows), rows)
