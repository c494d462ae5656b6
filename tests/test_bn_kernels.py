"""The plain BatchNorm chain of csrc/bn.hip (sgx_channel_stats_partial, sgx_bn_finalize, sgx_affine_act_fwd, sgx_bn_bwd_reduce, sgx_bn_bwd_finalize,
sgx_bn_bwd_apply, sgx_relu_bwd, sgx_relu_bwd_bn_reduce, the synchronised-BatchNorm entries sgx_bn_reduce_sums, sgx_bn_finalize_sums,
sgx_bn_bwd_finalize_sums, and sgx_dot / sgx_axpy / sgx_colsum on the same sweep skeleton) against plain torch in fp64 with autograd on the same
fp32 operands, as [M, C] matrices:  pre = (x - mean) / sqrt(var_biased + eps) * gamma + beta,  y = act(pre + a1 * r1 + a2 * r2),  y.backward(dy);
the running statistics with momentum 0.03 and the unbiased variance.  The shapes walk the launch geometries no whole-network test reaches:
several channel strips with a part-filled last one, channel counts whose float4 groups do not divide the workgroup, fewer rows than row lanes,
row blocks longer than 64 rows (sgx_stats_blocks at its cap) and every form of the finalize.  Both back ends run the same shapes; every case
first asserts, from the library's own size queries, the geometry it was chosen for.

Bars.  On the well-conditioned inputs (x ~ N(0.5, 2^2)) a quantity's bar is min(project bar, max(4 * e32, 2^-21)): e32 is the distance of fp32
ATen on the CPU (torch.native_batch_norm + autograd, or the plain fp32 torch expression) from the same fp64 reference on the same operands -
the kernels do the same arithmetic in another summation order, and the chip's expf and fma contraction may differ (the factor 4); 2^-21 is
4 ulp at the tensor's max-abs, because e32 can be next to 0 by luck on a small tensor.  The project bars: 2e-5 element-wise results and rows,
5e-5 dx / dgamma / dbeta, 1e-4 raw partial-row sums.  A bar is computed from the references, never from the kernel.

Every comparison prints `BN_ERR <kernel> <quantity> <bar> <measured>` before it asserts (pytest -rP shows the lines).
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from util import rel_err

from super_gradients_amd import kernels as K
from super_gradients_amd._lib import SgxError
from test_qarep_kernels import CR_COOP_MAX, CR_DIRECT, CR_MAX_SLICES, LAYOUTS, NAN, SW_MAXCG, SW_THREADS, _Guard, _bits, _mat, _result, _rows, _same_bits, _seed

TOL = 2e-5         # element-wise results and per-channel rows, of the tensor's max-abs (tests/test_kernels.py)
TOL_GRAD = 5e-5    # dx, dgamma, dbeta (tests/test_kernels.py::test_batchnorm_train)
TOL_PART = 1e-4    # raw partial-row sums and column sums (tests/test_kernels.py)
TOL_FORMS = 2e-6   # one finalize form against another (tests/test_kernels.py::test_fused_finalize)
FLOOR = 2.0 ** -21  # 4 ulp at the tensor's max-abs
KINK = 1e-3        # no fp64 pre-activation lies this close to a kink of its activation
EPS, MOM = 1e-3, 0.03

ACTS = {"none": lambda t: t, "relu": F.relu, "silu": F.silu, "relu6": F.relu6, "hswish": F.hardswish}
KINKS = {"none": (), "silu": (), "relu": (0.0,), "relu6": (0.0, 6.0), "hswish": (-3.0, 3.0)}

# M rows, C channels; the channel geometry of the sweeps (strips, float4 groups of the last strip, row lanes), the partial rows
# (sgx_stats_blocks(M)), the rows of one block and the form the finalize over those partial rows takes
CASES = [
    # two strips, the last with two live groups; blocks of 57 rows on 4 row lanes: the 4-row unrolled loop (rows 0..47 of a lane's 15) and its tail
    SimpleNamespace(M=225, C=264, strips=2, last=2, RL=4, nblk=4, per=57, form="direct"),
    # blocks of 60 rows on 4 row lanes: the row after lane 0's last full 4-row group (row 48 + 3 x 4 = 60) is the next block's first row -
    # an unrolled loop that ran on `<=` would add it to this block's partial rows too (the last block has 57 rows: nothing past the tensor)
    SimpleNamespace(M=237, C=264, strips=2, last=2, RL=4, nblk=4, per=60, form="direct"),
    # C / 4 = 18: RL = 14, 252 live lanes
    SimpleNamespace(M=529, C=72, strips=1, last=18, RL=14, nblk=9, per=59, form="direct"),
    # one channel group, 256 row lanes, blocks shorter than RL
    SimpleNamespace(M=513, C=4, strips=1, last=1, RL=256, nblk=9, per=57, form="direct"),
    # five strips, the last with one live group; M < the rows of one block (and a second row in two of the four row lanes only)
    SimpleNamespace(M=9, C=1028, strips=5, last=1, RL=4, nblk=1, per=9, form="direct"),
    # strips of 64 + 30 groups
    SimpleNamespace(M=392, C=376, strips=2, last=30, RL=4, nblk=7, per=56, form="direct"),
    # 33 partial rows: the first cooperative finalize, forward and backward
    SimpleNamespace(M=2100, C=8, strips=1, last=2, RL=128, nblk=33, per=64, form="coop"),
    # sgx_stats_blocks at its cap: 65-row blocks on 256 lanes (the last 14 blocks empty); 1024 partial rows reach the 16-row unrolled loop of col_lane_sums
    SimpleNamespace(M=65601, C=4, strips=1, last=1, RL=256, nblk=1024, per=65, form="coop"),
]
CASE_IDS = [f"{c.M}x{c.C}" for c in CASES]
BY_SHAPE = {(c.M, c.C): c for c in CASES}


def _finalize_form(nblk, C):
    """Which form a two-plane finalize over nblk partial rows takes, read off sgx_reduce_workspace (2 planes x slices x C doubles + 256)."""
    ws = K.lib().sgx_reduce_workspace(nblk, C) - 256
    assert ws % (2 * C * 8) == 0
    slices = ws // (2 * C * 8)
    if slices == 0:
        assert nblk <= CR_DIRECT
        return "direct"
    assert nblk > CR_DIRECT and slices == min(CR_MAX_SLICES, -(-nblk // 32))
    return "coop" if nblk <= CR_COOP_MAX else "two-launch"


def _assert_geometry(case):
    """The geometry the case claims: a change of the row-block rule or of the finalize thresholds fails here."""
    c4 = case.C // 4
    cg = min(c4, SW_MAXCG)
    strips = -(-c4 // cg)
    assert (strips, c4 - (strips - 1) * cg, SW_THREADS // cg) == (case.strips, case.last, case.RL)
    assert K.stats_blocks(case.M) == case.nblk and -(-case.M // case.nblk) == case.per
    assert K.lib().sgx_dot_workspace(case.M, case.C) == case.nblk * case.strips * 8 + 256
    assert _finalize_form(case.nblk, case.C) == case.form
    assert K.lib().sgx_bn_get_fused_finalize() == 1


# --------------------------------------------------------------------------------------------- references and comparisons
def _bar(project, e32):
    return min(project, max(4.0 * e32, FLOOR))


def _close(got, ref, bar, kernel, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.numel() == ref.numel(), f"{kernel} {what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    got = got.reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    e = rel_err(got, ref)
    print(f"BN_ERR {kernel} {what} {bar:.3g} {e:.3e}")
    assert e <= bar, f"{kernel} {what}: max err {e:.3e} of the tensor's max-abs > {bar:.3g}"
    return e


def _block_sums(t, nblk, dtype=torch.float64):
    """[nblk, C] sums of a [M, C] matrix over ceil(M / nblk) consecutive rows per block (empty blocks: 0), accumulated in `dtype`."""
    m, c = t.shape
    per = -(-m // nblk)
    padded = torch.zeros(nblk * per, c, dtype=dtype)
    padded[:m] = t.to(dtype)
    return padded.view(nblk, per, c).sum(1)


def _away_from_kinks(x, pre_of, step_of, act):
    """x nudged until no fp64 pre-activation pre_of(x) lies within KINK of a kink of act: an offending element of x moves by
    4 * KINK in pre-activation units (step_of(): d x per unit of pre, per channel), away from the kink.  -> x; asserts the margin."""
    for rounds in range(11):
        pre = pre_of(x)
        bad = torch.zeros_like(pre, dtype=torch.bool)
        sign = torch.zeros_like(pre)
        for k in KINKS[act]:
            near = (pre - k).abs() < KINK
            sign = torch.where(near, torch.where(pre >= k, 1.0, -1.0).to(pre.dtype), sign)
            bad |= near
        if not bool(bad.any()):
            break
        assert rounds < 10, f"{act}: pre-activations within KINK of a kink after 10 rounds"
        x = torch.where(bad, (x.double() + sign * 4 * KINK * step_of()).float(), x)
    for k in KINKS[act]:
        assert float((pre - k).abs().min()) >= KINK
        assert bool((pre < k).any()) and bool((pre > k).any()), f"{act}: no pre-activation on one side of {k}"
    return x


def _bn_reference(x, gamma, beta, dy, act):
    """fp64 autograd on the fp32 operands."""
    xd, w, b = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    pre = (xd - mean) / torch.sqrt(var + EPS) * w + b
    pre.retain_grad()
    ACTS[act](pre).backward(dy.double())
    with torch.no_grad():
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = w * invstd
        return SimpleNamespace(y=ACTS[act](pre), pre=pre.detach(), dx=xd.grad, g=pre.grad, dgamma=w.grad, dbeta=b.grad, save_mean=mean.detach(),
                               save_invstd=invstd, var=var.detach(), scale=scale, shift=b - mean * scale)


def _bn_aten32(x, gamma, beta, rm, rv, dy, act):
    """The same in fp32 by ATen on the CPU: torch.native_batch_norm (which also returns save_mean / save_invstd) plus autograd."""
    x32, w, b = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.clone(), rv.clone()
    pre, mean, invstd = torch.native_batch_norm(x32, w, b, rm, rv, True, MOM, EPS)
    pre.retain_grad()
    y = ACTS[act](pre)
    y.backward(dy)
    with torch.no_grad():
        scale = w * invstd
        return SimpleNamespace(y=y.detach(), dx=x32.grad, g=pre.grad, dgamma=w.grad, dbeta=b.grad, save_mean=mean, save_invstd=invstd, scale=scale,
                               shift=b - mean * scale, running_mean=rm, running_var=rv)


QUANTITIES = {"y": TOL, "g": TOL, "scale": TOL, "shift": TOL, "save_mean": TOL, "save_invstd": TOL, "running_mean": TOL, "running_var": TOL,
              "dx": TOL_GRAD, "dgamma": TOL_GRAD, "dbeta": TOL_GRAD, "sum": TOL_PART, "sumsq": TOL_PART}


def _make_case(M, C, act, x, dy, g):
    """The references of one input (x, dy): fp64, fp32 ATen, and per quantity e32 and the bar."""
    rn, ru = lambda *s: torch.randn(*s, generator=g), lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    gamma, beta = 2.0 * (ru(C) + 0.5), rn(C)
    rm, rv = rn(C), ru(C) + 0.5
    start = SimpleNamespace(dgamma=rn(C), dbeta=rn(C))
    x = _away_from_kinks(x, lambda t: _bn_reference(t, gamma, beta, dy, act).pre, lambda: 1.0 / _bn_reference(x, gamma, beta, dy, act).scale, act)
    ref = _bn_reference(x, gamma, beta, dy, act)
    ref.running_mean = (1 - MOM) * rm.double() + MOM * ref.save_mean
    ref.running_var = (1 - MOM) * rv.double() + MOM * ref.var * (M / (M - 1.0))
    nblk = K.stats_blocks(M)
    xd = x.double()
    ref.sum, ref.sumsq = _block_sums(xd, nblk), _block_sums(xd * xd, nblk)
    a32 = _bn_aten32(x, gamma, beta, rm, rv, dy, act)
    a32.sum, a32.sumsq = _block_sums(x, nblk, torch.float32), _block_sums(x * x, nblk, torch.float32)
    e32 = {q: rel_err(getattr(a32, q), getattr(ref, q)) for q in QUANTITIES}
    bar = {q: _bar(QUANTITIES[q], e32[q]) for q in QUANTITIES}
    return SimpleNamespace(M=M, C=C, act=act, x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, start=start, ref=ref, a32=a32, e32=e32, bar=bar)


@functools.lru_cache(maxsize=None)
def _case(M, C, act):
    """Inputs and references, built once per case and shared by both back ends and both layouts (nothing here is written afterwards):
    x ~ N(0.5, 2^2) with a per-channel offset, gamma in 1..3 so that relu6 and hard-swish see all their pieces."""
    g = torch.Generator().manual_seed(_seed(M, C, act))
    x = 2.0 * torch.randn(M, C, generator=g) + 0.5 + 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g) + 0.5 * torch.randn(C, generator=g)
    return _make_case(M, C, act, x, dy, g)


# --------------------------------------------------------------------------------------------- the launches, through lib()
def _stats(xk):
    M, C = xk.shape[2], xk.shape[3]
    nb = K.stats_blocks(M)
    parts = _rows(None, xk.device, 2 * nb, C).view(2, nb, C)
    guard = _Guard("channel_stats_partial", partials=parts)
    K.check(K.lib().sgx_channel_stats_partial(K.ptr(xk), M, C, K.rows(xk)[1], K.ptr(parts), K.stream()), "sgx_channel_stats_partial")
    guard.check()
    return parts


def _finalize(cs, parts, M, dev):
    """sgx_bn_finalize into guarded NaN-filled rows and guarded copies of the running statistics."""
    nb, C = parts.shape[1], parts.shape[2]
    L = K.lib()
    o = SimpleNamespace(scale=_rows(None, dev, None, C), shift=_rows(None, dev, None, C), save_mean=_rows(None, dev, None, C), save_invstd=_rows(None, dev, None, C),
                        running_mean=_rows(cs.rm, dev), running_var=_rows(cs.rv, dev))
    gamma, beta = cs.gamma.to(dev), cs.beta.to(dev)
    ws = K.WORKSPACE.get(L.sgx_reduce_workspace(nb, C), dev)
    guard = _Guard("bn_finalize", **vars(o))
    K.check(L.sgx_bn_finalize(K.ptr(parts), nb, M, C, K.ptr(gamma), K.ptr(beta), EPS, MOM, K.ptr(o.running_mean), K.ptr(o.running_var), K.ptr(o.save_mean),
                              K.ptr(o.save_invstd), K.ptr(o.scale), K.ptr(o.shift), K.ptr(ws), ws.numel(), K.stream()), "sgx_bn_finalize")
    guard.check()
    return o


def _bwd_reduce(dk, xk, f, act):
    M, C = xk.shape[2], xk.shape[3]
    nb = K.stats_blocks(M)
    parts = _rows(None, xk.device, 2 * nb, C).view(2, nb, C)
    guard = _Guard("bn_bwd_reduce", partials=parts)
    K.check(K.lib().sgx_bn_bwd_reduce(K.ptr(dk), K.rows(dk)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(f.scale), K.ptr(f.shift), K.ptr(f.save_mean), M, C, K.ACT[act],
                                      K.ptr(parts), K.stream()), "sgx_bn_bwd_reduce")
    guard.check()
    return parts


def _bwd_finalize(cs, parts, M, save_mean, save_invstd, dev):
    """sgx_bn_bwd_finalize onto guarded copies of the non-zero starting gradients, coef guarded and NaN-filled."""
    nb, C = parts.shape[1], parts.shape[2]
    L = K.lib()
    o = SimpleNamespace(coef=_rows(None, dev, 5, C), dgamma=_rows(cs.start.dgamma, dev), dbeta=_rows(cs.start.dbeta, dev))
    gamma = cs.gamma.to(dev)
    ws = K.WORKSPACE.get(L.sgx_reduce_workspace(nb, C), dev)
    guard = _Guard("bn_bwd_finalize", **vars(o))
    K.check(L.sgx_bn_bwd_finalize(K.ptr(parts), nb, M, C, K.ptr(gamma), K.ptr(save_mean), K.ptr(save_invstd), K.ptr(o.dgamma), K.ptr(o.dbeta), K.ptr(o.coef), K.ptr(ws),
                                  ws.numel(), K.stream()), "sgx_bn_bwd_finalize")
    guard.check()
    return o


def _bwd_apply(dk, xk, f, coef, act, dx, g):
    M, C = xk.shape[2], xk.shape[3]
    guard = _Guard("bn_bwd_apply", dx=dx, **({} if g is None else dict(g=g)))
    K.check(K.lib().sgx_bn_bwd_apply(K.ptr(dk), K.rows(dk)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(f.scale), K.ptr(f.shift), K.ptr(coef), K.ptr(dx), K.rows(dx)[1], K.ptr(g),
                                     K.rows(g)[1] if g is not None else 0, M, C, K.ACT[act], K.stream()), "sgx_bn_bwd_apply")
    guard.check()


def _grads(cs, b):
    return {k: getattr(b, k).cpu().double() - getattr(cs.start, k).double() for k in ("dgamma", "dbeta")}


def _chain(cs, dev, layout, quantities=None):
    """The whole chain, launch by launch, every output in guarded NaN-filled memory, against cs.ref at cs.bar -> the outputs and the errors."""
    M, C, act, ref = cs.M, cs.C, cs.act, cs.ref
    err = {}

    def close(got, q, kernel):
        print(f"BN_ERR fp32-ATen {q}[{act}] - {cs.e32[q]:.3e}")
        if quantities is None or q in quantities:
            err[q] = _close(got, getattr(ref, q), cs.bar[q], kernel, f"{q}[{act}]")
        else:  # (printed, not asserted)
            print(f"BN_ERR {kernel} {q}[{act}] - {rel_err(got.detach().cpu().reshape(getattr(ref, q).shape), getattr(ref, q)):.3e}")

    xk, dk = _mat(cs.x, dev, layout, 0), _mat(cs.dy, dev, layout, 1)
    xbits, dbits = _bits(xk), _bits(dk)
    parts = _stats(xk)
    close(parts[0], "sum", "channel_stats_partial")
    close(parts[1], "sumsq", "channel_stats_partial")
    f = _finalize(cs, parts, M, dev)
    for q in ("scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var"):
        close(getattr(f, q), q, "bn_finalize")
    y = _result(M, C, dev, layout, 2)
    guard = _Guard("affine_act", y=y)
    assert K.affine_act(xk, f.scale, f.shift, act=act, out=y) is y
    guard.check()
    close(y, "y", "affine_act_fwd")
    bparts = _bwd_reduce(dk, xk, f, act)
    b = _bwd_finalize(cs, bparts, M, f.save_mean, f.save_invstd, dev)
    dx, g = _result(M, C, dev, layout, 3), _result(M, C, dev, layout, 4)
    _bwd_apply(dk, xk, f, b.coef, act, dx, g)
    assert torch.equal(_bits(xk), xbits) and torch.equal(_bits(dk), dbits), "the out-of-place chain changed its inputs"
    close(dx, "dx", "bn_bwd_apply")
    close(g, "g", "bn_bwd_apply")
    for q, got in _grads(cs, b).items():
        close(got, q, "bn_bwd_finalize")
    return SimpleNamespace(xk=xk, dk=dk, parts=parts, f=f, y=y, bparts=bparts, b=b, dx=dx, g=g, err=err)


# --------------------------------------------------------------------------------------------- 1. the chain against fp64
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bn_chain(backend, case, act, layout):
    """Statistics partials per partial row, the finalize's six rows, y, dx, g, dgamma / dbeta (onto non-zero starting values) against fp64
    autograd; nothing written outside an output.  K.bn_bwd (the wrapper the layers call, want_g) gives the bits of the three launches."""
    _assert_geometry(case)
    cs = _case(case.M, case.C, act)
    dev = backend
    r = _chain(cs, dev, layout)
    dgamma, dbeta = _rows(cs.start.dgamma, dev), _rows(cs.start.dbeta, dev)
    guard = _Guard("bn_bwd", dgamma=dgamma, dbeta=dbeta)
    dx, g = K.bn_bwd(r.dk, r.xk, r.f.scale, r.f.shift, cs.gamma.to(dev), r.f.save_mean, r.f.save_invstd, dgamma, dbeta, act=act, want_g=True)
    guard.check()
    assert _same_bits(dx, r.dx) and _same_bits(g, r.g) and _same_bits(dgamma, r.b.dgamma) and _same_bits(dbeta, r.b.dbeta), "K.bn_bwd differs from the three launches"


@functools.lru_cache(maxsize=None)
def _affine_case(M, C):
    g = torch.Generator().manual_seed(_seed(M, C, "affine"))
    rn, ru = lambda *s: torch.randn(*s, generator=g), lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    return SimpleNamespace(x=2.0 * rn(M, C) + 0.5, r1=rn(M, C), r2=rn(M, C) + rn(C), scale=ru(C) + 0.5, shift=rn(C))


# (name, scale / shift given, r1, a1 through the device scalar, r2, statistics, activation)
AFFINE = [("r1-host-a1", True, True, False, False, False, "relu6"), ("r1-a1_dev", True, True, True, False, False, "hswish"),
          ("r1-r2-stats", True, True, False, True, True, "silu"), ("no-scale-r1", False, True, True, False, False, "relu"),
          ("r2-only-stats", True, False, False, True, True, "none")]
A1, A2 = 0.7, 1.5


@functools.lru_cache(maxsize=None)
def _affine_variant(M, C, name):
    _, scaled, has_r1, _, has_r2, _, act = next(v for v in AFFINE if v[0] == name)
    o = _affine_case(M, C)
    sc, sh = (o.scale, o.shift) if scaled else (torch.ones(C), torch.zeros(C))

    def pre_of(x, dt=torch.float64):
        v = sc.to(dt) * x.to(dt) + sh.to(dt)
        if has_r1:
            v = v + torch.tensor(A1, dtype=torch.float32).to(dt) * o.r1.to(dt)
        if has_r2:
            v = v + A2 * o.r2.to(dt)
        return v

    x = _away_from_kinks(o.x, pre_of, lambda: 1.0 / sc.double(), act)
    pre = pre_of(x)
    pre32 = pre_of(x, torch.float32)
    nblk = K.stats_blocks(M)
    ref = SimpleNamespace(y=ACTS[act](pre), sum=_block_sums(pre, nblk), sumsq=_block_sums(pre * pre, nblk))
    a32 = SimpleNamespace(y=ACTS[act](pre32), sum=_block_sums(pre32, nblk, torch.float32), sumsq=_block_sums(pre32 * pre32, nblk, torch.float32))
    bar = {q: _bar(QUANTITIES[q], rel_err(getattr(a32, q), getattr(ref, q))) for q in ("y", "sum", "sumsq")}
    return SimpleNamespace(x=x, ref=ref, bar=bar)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", AFFINE, ids=[v[0] for v in AFFINE])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_affine_act(backend, case, variant, layout):
    """sgx_affine_act_fwd on its own: y = act(scale * x + shift + a1 * r1 + a2 * r2) with r1 scaled by the host a1 or by the device scalar
    (the host value then being ignored), r2, scale = NULL (y = act(x + ...)) and the statistics rows of the pre-activation."""
    _assert_geometry(case)
    name, scaled, has_r1, dev_a1, has_r2, stats, act = variant
    M, C, dev = case.M, case.C, backend
    o, v = _affine_case(M, C), _affine_variant(M, C, name)
    xk = _mat(v.x, dev, layout, 0)
    r1 = _mat(o.r1, dev, layout, 1) if has_r1 else None
    r2 = _mat(o.r2, dev, layout, 2) if has_r2 else None
    y = _result(M, C, dev, layout, 3)
    nb = K.stats_blocks(M)
    parts = _rows(None, dev, 2 * nb, C).view(2, nb, C) if stats else None
    a1_dev = torch.tensor([A1], device=dev) if dev_a1 else None
    scale, shift = (o.scale.to(dev), o.shift.to(dev)) if scaled else (None, None)
    guard = _Guard("affine_act", y=y, **(dict(partials=parts) if stats else {}))
    K.check(K.lib().sgx_affine_act_fwd(K.ptr(xk), K.rows(xk)[1], K.ptr(scale), K.ptr(shift), K.ptr(r1), K.rows(r1)[1] if has_r1 else 0, 123.0 if dev_a1 else A1,
                                       K.ptr(a1_dev), K.ptr(r2), K.rows(r2)[1] if has_r2 else 0, A2, K.ptr(y), K.rows(y)[1], M, C, K.ACT[act], K.ptr(parts), K.stream()),
            "sgx_affine_act_fwd")
    guard.check()
    _close(y, v.ref.y, v.bar["y"], "affine_act_fwd", f"y[{name},{act}]")
    if stats:
        _close(parts[0], v.ref.sum, v.bar["sum"], "affine_act_fwd", f"sum[{name}]")
        _close(parts[1], v.ref.sumsq, v.bar["sumsq"], "affine_act_fwd", f"sumsq[{name}]")
        yw, pw = K.affine_act(xk, scale, shift, r1=r1, a1=A1, a1_dev=a1_dev, r2=r2, a2=A2, act=act, want_stats=True)
        assert _same_bits(yw, y) and _same_bits(pw, parts), "K.affine_act differs from the direct call"


# --------------------------------------------------------------------------------------------- 2. the finalize forms
FORM_ROWS = [(1, 72), (32, 12), (33, 12), (300, 12), (1000, 8), (1024, 12), (4096, 8), (4200, 12)]


def _per(nblk):
    """Rows of x behind every synthetic partial row: 3, and more while the batch would have fewer than 96 rows (the variance of a handful of
    rows can be far below mean^2, which is the conditioning test's subject, not this one's)."""
    return max(3, -(-96 // nblk))


@functools.lru_cache(maxsize=None)
def _forms_case(nblk, C):
    """Synthetic partial rows, free of M: fp64 block sums over _per(nblk) rows each, rounded once to fp32 - for the forward finalize sum x, sum x^2;
    for the backward sum g, sum g (x - mean) with g = dy and mean the fp32 save_mean the kernel is handed."""
    M = _per(nblk) * nblk
    g = torch.Generator().manual_seed(_seed(nblk, C, "forms"))
    x = 2.0 * torch.randn(M, C, generator=g) + 0.5 + 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g) + 0.5 * torch.randn(C, generator=g)
    cs = _make_case(M, C, "none", x, dy, g)
    xd, gd = x.double(), dy.double()
    cs.fwd_parts = torch.stack([_block_sums(xd, nblk), _block_sums(xd * xd, nblk)]).float()
    cs.mean32, cs.invstd32 = cs.ref.save_mean.float(), cs.ref.save_invstd.float()
    cs.bwd_parts = torch.stack([_block_sums(gd, nblk), _block_sums(gd * (xd - cs.mean32.double()), nblk)]).float()
    # the coefficient rows are functions of the operands the kernel is handed - the fp32 save_mean / save_invstd, sums centred on that mean
    sgx, inv = (gd * (xd - cs.mean32.double())).sum(0), cs.invstd32.double()
    cs.coef = torch.stack([cs.gamma.double() * inv, gd.mean(0), inv * inv * sgx / M, cs.mean32.double()])
    return cs


def _run_forms(cs, nblk, C, dev):
    """Both finalizes on the synthetic rows -> every output, on the CPU."""
    f = _finalize(cs, cs.fwd_parts.to(dev), cs.M, dev)
    b = _bwd_finalize(cs, cs.bwd_parts.to(dev), cs.M, cs.mean32.to(dev), cs.invstd32.to(dev), dev)
    out = {**{k: v for k, v in vars(f).items()}, "dgamma": b.dgamma, "dbeta": b.dbeta, **{f"coef:{k}": b.coef[k] for k in range(5)}}
    return {k: v.cpu().clone() for k, v in out.items()}


def _check_forms(cs, r, tag):
    for q in ("scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var"):
        _close(r[q], getattr(cs.ref, q), cs.bar[q], "bn_finalize", f"{q}[{tag}]")
    for q in ("dgamma", "dbeta"):
        _close(r[q].double() - getattr(cs.start, q).double(), getattr(cs.ref, q), cs.bar[q], "bn_bwd_finalize", f"{q}[{tag}]")
    # coef rows: c1 = gamma * invstd, mean g as hi + lo floats, k = invstd^2 * mean(g (x - mean)), the mean handed in: fp64 arithmetic on the
    # operands, rounded once - the bar is the floor, 4 ulp
    for k, (name, got) in enumerate((("c1", r["coef:0"].double()), ("mean-g", r["coef:1"].double() + r["coef:4"].double()), ("k", r["coef:2"].double()),
                                     ("mean", r["coef:3"].double()))):
        _close(got, cs.coef[k], FLOOR, "bn_bwd_finalize", f"coef:{name}[{tag}]")
    assert float((r["coef:4"].double().abs() / r["coef:1"].double().abs().clamp_min(1e-30)).max()) <= 2.0 ** -24, "coef row 4 is the low word of mean g"


@pytest.mark.parametrize("nblk,C", FORM_ROWS, ids=[f"{n}x{c}" for n, c in FORM_ROWS])
def test_bn_finalize_forms(backend, nblk, C):
    """sgx_bn_finalize and sgx_bn_bwd_finalize over 1 .. 4200 partial rows against fp64 truth: direct (up to 32 rows), cooperative (33 .. 4096;
    1000 rows leave the 16-row unrolled loop of col_lane_sums live for the row lanes below 40 only) and, above 4096, the two-launch form
    through colreduce_kernel<2>.  300 and 4200 rows run again with sgx_bn_set_fused_finalize(0) - the pre-reduction and the one-thread-per-
    channel finalize - and the forms agree to 2e-6."""
    L, dev = K.lib(), backend
    form = _finalize_form(nblk, C)
    assert form == ("direct" if nblk <= 32 else "coop" if nblk <= 4096 else "two-launch")
    cs = _forms_case(nblk, C)
    assert L.sgx_bn_get_fused_finalize() == 1
    fused = _run_forms(cs, nblk, C, dev)
    _check_forms(cs, fused, form)
    if nblk not in (300, 4200):
        return
    prev = L.sgx_bn_get_fused_finalize()
    try:
        L.sgx_bn_set_fused_finalize(0)
        plain = _run_forms(cs, nblk, C, dev)
    finally:
        L.sgx_bn_set_fused_finalize(prev)
    assert L.sgx_bn_get_fused_finalize() == 1
    _check_forms(cs, plain, "switch-off")
    for k in fused:
        _close(fused[k], plain[k].double(), TOL_FORMS, "bn_finalize" if k in QUANTITIES and k not in ("dgamma", "dbeta") else "bn_bwd_finalize", f"forms:{k}")


COLSUM_ROWS = [1, 32, 33, 300, 1000, 1024]  # (sgx_colsum's partial rows are sgx_stats_blocks(M) <= 1024: the larger counts are out of its reach)


@functools.lru_cache(maxsize=None)
def _colsum_case(M, C):
    g = torch.Generator().manual_seed(_seed(M, C, "colsum"))
    x = torch.randn(M, C, generator=g) + 0.5 * torch.randn(C, generator=g)
    start = torch.randn(C, generator=g)
    ref = x.double().sum(0)
    return SimpleNamespace(x=x, start=start, ref=ref, bar=_bar(TOL_PART, rel_err(x.sum(0), ref)))


@pytest.mark.parametrize("nblk", COLSUM_ROWS)
def test_colsum_row_counts(backend, nblk):
    """sgx_colsum with 1 .. 1024 partial rows of its own sweep (M = 64 * nblk - 5) against the fp64 column sums, accumulated onto non-zero
    values; 300 rows again with the fused switch off: the forms agree to 2e-6."""
    L, dev, C = K.lib(), backend, 12
    M = 64 * nblk - 5
    assert K.stats_blocks(M) == nblk
    cs = _colsum_case(M, C)
    xk = _mat(cs.x, dev, "contiguous", 0)
    res = {}
    prev = L.sgx_bn_get_fused_finalize()
    try:
        for fused in (1, 0) if nblk == 300 else (1,):
            L.sgx_bn_set_fused_finalize(fused)
            out = _rows(cs.start, dev)
            guard = _Guard("colsum", out=out)
            K.colsum(xk, out, accumulate=True)
            guard.check()
            res[fused] = out.cpu().double() - cs.start.double()
            _close(res[fused], cs.ref, cs.bar, "colsum", f"rows={nblk}[fused={fused}]")
    finally:
        L.sgx_bn_set_fused_finalize(prev)
    assert L.sgx_bn_get_fused_finalize() == 1
    if nblk == 300:
        _close(res[1], res[0], TOL_FORMS, "colsum", "forms")


# --------------------------------------------------------------------------------------------- 3. two simulated ranks
def _reduce_sums(parts, dev):
    nb, C = parts.shape[1], parts.shape[2]
    sums = torch.full((2 * C + 64,), NAN, dtype=torch.float64, device=dev)
    ws = K.WORKSPACE.get(K.lib().sgx_reduce_workspace(nb, C), dev)
    K.check(K.lib().sgx_bn_reduce_sums(K.ptr(parts), nb, C, K.ptr(sums[32:]), K.ptr(ws), ws.numel(), K.stream()), "sgx_bn_reduce_sums")
    assert bool(torch.isnan(sums[:32]).all()) and bool(torch.isnan(sums[32 + 2 * C:]).all()), "bn_reduce_sums wrote outside its sums"
    return sums[32:32 + 2 * C].view(2, C).cpu()


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_bn_two_ranks(backend, act):
    """Synchronised BatchNorm without torch.distributed: the 2100 rows as two ranks of 1000 + 1100.  Forward: statistics partials and
    sgx_bn_reduce_sums per half, the fp64 sums added on the host, sgx_bn_finalize_sums with the total row count - the whole batch's fp64
    statistics, and within 2e-6 of the unsynchronised finalize.  Backward: sgx_bn_bwd_reduce and sgx_bn_reduce_sums per half (the local
    sums), their sum (the global sums), sgx_bn_bwd_finalize_sums and the apply per half: the concatenated dx is the whole batch's, each
    half's dgamma / dbeta the fp64 sum over that half's rows only - the one place where the two kinds of sums can be mixed up."""
    case = BY_SHAPE[(2100, 8)]
    _assert_geometry(case)
    M, C, dev, L = case.M, case.C, backend, K.lib()
    cs = _case(M, C, act)
    ref, a32 = cs.ref, cs.a32
    halves = [(0, 1000), (1000, 2100)]
    xk, dk = _mat(cs.x, dev, "slices", 0), _mat(cs.dy, dev, "slices", 1)
    xs, ds = [xk[:, :, a:b] for a, b in halves], [dk[:, :, a:b] for a, b in halves]
    assert [K.stats_blocks(b - a) for a, b in halves] == [16, 18]
    gamma, beta = cs.gamma.to(dev), cs.beta.to(dev)

    # forward
    total = sum(_reduce_sums(_stats(x), dev) for x in xs)
    _close(total[0], cs.x.double().sum(0), cs.bar["sum"], "bn_reduce_sums", "sum")
    _close(total[1], (cs.x.double() ** 2).sum(0), cs.bar["sumsq"], "bn_reduce_sums", "sumsq")
    f = SimpleNamespace(scale=_rows(None, dev, None, C), shift=_rows(None, dev, None, C), save_mean=_rows(None, dev, None, C), save_invstd=_rows(None, dev, None, C),
                        running_mean=_rows(cs.rm, dev), running_var=_rows(cs.rv, dev))
    guard = _Guard("bn_finalize_sums", **vars(f))
    sums = total.to(dev)
    K.check(L.sgx_bn_finalize_sums(K.ptr(sums), M, C, K.ptr(gamma), K.ptr(beta), EPS, MOM, K.ptr(f.running_mean), K.ptr(f.running_var), K.ptr(f.save_mean),
                                   K.ptr(f.save_invstd), K.ptr(f.scale), K.ptr(f.shift), K.stream()), "sgx_bn_finalize_sums")
    guard.check()
    whole = _finalize(cs, _stats(xk), M, dev)
    for q in vars(f):
        _close(getattr(f, q), getattr(ref, q), cs.bar[q], "bn_finalize_sums", f"{q}[{act}]")
        _close(getattr(f, q), getattr(whole, q).cpu().double(), TOL_FORMS, "bn_finalize_sums", f"{q}[{act}] vs bn_finalize")

    # backward
    local = [_reduce_sums(_bwd_reduce(d, x, f, act), dev) for d, x in zip(ds, xs)]
    glob = (local[0] + local[1]).to(dev)
    xhat, xhat32 = (cs.x.double() - ref.save_mean) * ref.save_invstd, (cs.x - a32.save_mean) * a32.save_invstd
    dxs, got = [], {"dgamma": [], "dbeta": []}
    for h, (a, b) in enumerate(halves):
        loc = local[h].to(dev)
        o = SimpleNamespace(coef=_rows(None, dev, 5, C), dgamma=_rows(cs.start.dgamma, dev), dbeta=_rows(cs.start.dbeta, dev))
        guard = _Guard("bn_bwd_finalize_sums", **vars(o))
        K.check(L.sgx_bn_bwd_finalize_sums(K.ptr(loc), K.ptr(glob), M, C, K.ptr(gamma), K.ptr(f.save_mean), K.ptr(f.save_invstd), K.ptr(o.dgamma), K.ptr(o.dbeta),
                                           K.ptr(o.coef), K.stream()), "sgx_bn_bwd_finalize_sums")
        guard.check()
        dx = _result(b - a, C, dev, "slices", 3 + h)
        _bwd_apply(ds[h], xs[h], f, o.coef, act, dx, None)
        dxs.append(dx.cpu().view(b - a, C))
        # this half's own gradient: the fp64 sums over its rows only; the bar from fp32 ATen's g and x-hat over the same rows
        own = {"dgamma": (ref.g[a:b] * xhat[a:b]).sum(0), "dbeta": ref.g[a:b].sum(0)}
        own32 = {"dgamma": (a32.g[a:b] * xhat32[a:b]).sum(0), "dbeta": a32.g[a:b].sum(0)}
        for q, v in _grads(cs, o).items():
            _close(v, own[q], _bar(TOL_GRAD, rel_err(own32[q], own[q])), "bn_bwd_finalize_sums", f"{q}[{act}] rank {h}")
            got[q].append(v)
    _close(torch.cat(dxs), ref.dx, cs.bar["dx"], "bn_bwd_apply", f"dx[{act}] two ranks")
    for q in got:
        _close(got[q][0] + got[q][1], getattr(ref, q), cs.bar[q], "bn_bwd_finalize_sums", f"{q}[{act}] both ranks")


# --------------------------------------------------------------------------------------------- 4. bits
def _wrapped_chain(cs, dev, layout, base, alias=None):
    """The chain through the wrappers the layers call -> its outputs.  alias: 'y' affine_act(out = x), 'dx-x' bn_bwd(dx_out = x),
    'dx-dy' bn_bwd(dx_out = dy) - on copies of their own."""
    act, C = cs.act, cs.C
    xk, dk = _mat(cs.x, dev, layout, base), _mat(cs.dy, dev, layout, base + 1)
    parts = K.channel_stats_partial(xk)
    rm, rv = cs.rm.clone().to(dev), cs.rv.clone().to(dev)
    scale, shift, mean, invstd = K.bn_finalize(parts, cs.M, cs.gamma.to(dev), cs.beta.to(dev), EPS, MOM, rm, rv)
    if alias == "y":
        xc = _mat(cs.x, dev, layout, base + 2)
        guard = _Guard("affine_act in place", y=xc)
        y = K.affine_act(xc, scale, shift, act=act, out=xc)
        guard.check()
    else:
        y = K.affine_act(xk, scale, shift, act=act)
    dgamma, dbeta = cs.start.dgamma.clone().to(dev), cs.start.dbeta.clone().to(dev)
    if alias in ("dx-x", "dx-dy"):
        xc, dc = _mat(cs.x, dev, layout, base + 2), _mat(cs.dy, dev, layout, base + 3)
        out = xc if alias == "dx-x" else dc
        guard = _Guard("bn_bwd in place", dx=out)
        dx, g = K.bn_bwd(dc, xc, scale, shift, cs.gamma.to(dev), mean, invstd, dgamma, dbeta, act=act, dx_out=out, want_g=True)
        guard.check()
        assert dx is out
    else:
        dx, g = K.bn_bwd(dk, xk, scale, shift, cs.gamma.to(dev), mean, invstd, dgamma, dbeta, act=act, want_g=True)
    return dict(parts=parts, scale=scale, shift=shift, save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv, y=y, dx=dx, g=g, dgamma=dgamma,
                dbeta=dbeta)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,act", [((225, 264), "hswish"), ((529, 72), "relu"), ((2100, 8), "silu")], ids=["225x264", "529x72", "2100x8"])
def test_bn_bits(backend, shape, act, layout):
    """A second run of the chain repeats every output's bits (the reductions have a fixed order, no atomics), and the in-place calls the
    layers rely on - affine_act(out = x), bn_bwd(dx_out = x) (modules/repvgg_block.py), bn_bwd(dx_out = dy), relu_bwd(out = dy),
    axpy(out = x, accumulate) - give the bits of the out-of-place calls: a row is read completely before it is written."""
    case = BY_SHAPE[shape]
    _assert_geometry(case)
    cs, dev = _case(case.M, case.C, act), backend
    first = _wrapped_chain(cs, dev, layout, 0)
    for k, v in _wrapped_chain(cs, dev, layout, 2).items():
        assert _same_bits(v, first[k]), f"a second run gives other bits in {k}"
    for alias, keys in (("y", ("y",)), ("dx-x", ("dx", "g", "dgamma", "dbeta")), ("dx-dy", ("dx", "g", "dgamma", "dbeta"))):
        r = _wrapped_chain(cs, dev, layout, 4, alias)
        for k in keys:
            assert _same_bits(r[k], first[k]), f"in place ({alias}): {k} differs from the out-of-place call"
    # relu_bwd over dy, axpy accumulating onto its own input
    yk, dk = first["y"], _mat(cs.dy, dev, layout, 0)
    g_ref = K.relu_bwd(dk, yk)
    assert torch.equal(g_ref.cpu().view(case.M, case.C), cs.dy * (yk.cpu().view(case.M, case.C) > 0))
    dc = _mat(cs.dy, dev, layout, 1)
    guard = _Guard("relu_bwd in place", g=dc)
    assert K.relu_bwd(dc, yk, out=dc) is dc
    guard.check()
    assert _same_bits(dc, g_ref), "relu_bwd(out = dy) differs from the out-of-place call"
    a_dev = torch.tensor([A1], device=dev)
    xk, z = _mat(cs.x, dev, layout, 2), _mat(cs.x, dev, layout, 3)
    K.axpy(xk, a_dev=a_dev, out=z, accumulate=True)
    xc = _mat(cs.x, dev, layout, 4)
    guard = _Guard("axpy in place", out=xc)
    K.axpy(xc, a_dev=a_dev, out=xc, accumulate=True)
    guard.check()
    assert _same_bits(xc, z), "axpy(out = x, accumulate) differs from the out-of-place call"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(225, 264), (529, 72)], ids=["225x264", "529x72"])
def test_relu_bwd_bn_reduce_strips(backend, shape, layout):
    """sgx_relu_bwd_bn_reduce is sgx_relu_bwd followed by sgx_bn_bwd_reduce(act = none), bit for bit (tests/test_kernels.py covers one full
    strip): two strips with a part-filled last one, and 252 live lanes."""
    case = BY_SHAPE[shape]
    _assert_geometry(case)
    M, C, dev = case.M, case.C, backend
    cs = _case(M, C, "relu")
    dk, xk, yk = _mat(cs.dy, dev, layout, 0), _mat(cs.x, dev, layout, 1), _mat(cs.ref.y.float(), dev, layout, 2)
    mean = _rows(cs.ref.save_mean.float(), dev)
    nb = K.stats_blocks(M)
    g, parts = _result(M, C, dev, layout, 3), _rows(None, dev, 2 * nb, C).view(2, nb, C)
    guard = _Guard("relu_bwd_bn_reduce", g=g, partials=parts)
    K.check(K.lib().sgx_relu_bwd_bn_reduce(K.ptr(dk), K.rows(dk)[1], K.ptr(yk), K.rows(yk)[1], K.ptr(xk), K.rows(xk)[1], K.ptr(mean), K.ptr(g), K.rows(g)[1], M, C,
                                           K.ptr(parts), K.stream()), "sgx_relu_bwd_bn_reduce")
    guard.check()
    g_ref = K.relu_bwd(dk, yk)
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    f = SimpleNamespace(scale=one, shift=zero, save_mean=mean)
    parts_ref = _bwd_reduce(g_ref, xk, f, "none")
    assert _same_bits(g, g_ref), "g differs from sgx_relu_bwd's"
    assert _same_bits(parts, parts_ref), "reduce partials differ from sgx_bn_bwd_reduce's"
    gw, pw = K.relu_bwd_bn_reduce(dk, yk, xk, mean)
    assert _same_bits(gw, g) and _same_bits(pw, parts)
    gd = (cs.dy * (cs.ref.y > 0)).double()
    _close(parts[0], _block_sums(gd, nb), TOL_PART, "relu_bwd_bn_reduce", "sum g")
    _close(parts[1], _block_sums(gd * (cs.x.double() - mean.cpu().double()), nb), TOL_PART, "relu_bwd_bn_reduce", "sum g (x - mean)")


# --------------------------------------------------------------------------------------------- 5. dot, axpy, colsum
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(225, 264), (9, 1028)], ids=["225x264", "9x1028"])
def test_dot_axpy_colsum_strips(backend, shape, layout):
    """sgx_dot (workspace index blockIdx.y * gridDim.x + blockIdx.x with two and five strips), sgx_axpy and sgx_colsum against fp64."""
    case = BY_SHAPE[shape]
    _assert_geometry(case)
    M, C, dev = case.M, case.C, backend
    o = _affine_case(M, C)
    xk, rk = _mat(o.x, dev, layout, 0), _mat(o.r2, dev, layout, 1)
    xd, rd = o.x.double(), o.r2.double()
    # dot: out = scale * <x, r>, then accumulated a second time
    out = _rows(torch.tensor([3.0]), dev)
    ref = 0.5 * (xd * rd).sum().view(1)
    bar = _bar(TOL_PART, rel_err(0.5 * (o.x * o.r2).sum().view(1), ref))
    guard = _Guard("dot", out=out)
    K.dot_sum(xk, rk, out, accumulate=False, scale=0.5)
    guard.check()
    _close(out, ref, bar, "dot", "scale * <x, r>")
    K.dot_sum(xk, rk, out, accumulate=True, scale=0.5)
    guard.check()
    _close(out, 2 * ref, bar, "dot", "accumulated")
    # axpy: z = a_dev * x, then z += 2 * r
    a_dev = torch.tensor([A1], device=dev)
    z = _result(M, C, dev, layout, 2)
    guard = _Guard("axpy", z=z)
    K.axpy(xk, a=123.0, a_dev=a_dev, out=z)
    guard.check()
    a1 = torch.tensor(A1).double()
    _close(z, a1 * xd, _bar(TOL, rel_err(torch.tensor(A1) * o.x, a1 * xd)), "axpy", "a_dev * x")
    K.axpy(rk, a=2.0, out=z, accumulate=True)
    guard.check()
    _close(z, a1 * xd + 2 * rd, _bar(TOL, rel_err(torch.tensor(A1) * o.x + 2 * o.r2, a1 * xd + 2 * rd)), "axpy", "a_dev * x + 2 r")
    # colsum onto non-zero values
    start = o.shift
    cs_out = _rows(start, dev)
    guard = _Guard("colsum", out=cs_out)
    K.colsum(xk, cs_out, accumulate=True)
    guard.check()
    _close(cs_out.cpu().double() - start.double(), xd.sum(0), _bar(TOL_PART, rel_err(o.x.sum(0), xd.sum(0))), "colsum", "column sums")
    K.colsum(xk, cs_out, accumulate=False)
    guard.check()
    _close(cs_out, xd.sum(0), _bar(TOL_PART, rel_err(o.x.sum(0), xd.sum(0))), "colsum", "column sums, no accumulate")


def test_colsum_blocks_straddle_images(backend):
    """sgx_colsum on a 4-D view (the bias gradients' use): 5 images of 5 x 7 pixels, 175 rows in 3 blocks of 59 - the blocks straddle the
    images - the image stride (40 rows of 12 floats) not rows x ld; the surroundings are NaN."""
    dev, C = backend, 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 35, C, generator=g) + torch.randn(C, generator=g)
    buf = torch.full((5, 40, 12), NAN, dtype=torch.float32, device=dev)
    v = buf[:, :35, 4:12]
    v.copy_(x.to(dev))
    v = v.unflatten(1, (5, 7))
    assert v.stride() == (480, 84, 12, 1) and K.nhwc_strides(v) == (12, 480) and K.stats_blocks(175) == 3
    out = _rows(None, dev, None, C)
    guard = _Guard("colsum", out=out)
    K.colsum(v, out, accumulate=False)
    guard.check()
    ref = x.double().sum((0, 1))
    _close(out, ref, _bar(TOL_PART, rel_err(x.sum((0, 1)), ref)), "colsum", "4-D view")


# --------------------------------------------------------------------------------------------- 6. conditioning of the one-pass variance
@functools.lru_cache(maxsize=None)
def _conditioning_case(mean):
    M, C = 2100, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, C, generator=g) * 0.3 + mean
    dy = torch.randn(M, C, generator=g) + 0.5 * torch.randn(C, generator=g)  # (that test's nearly constant dy makes dx pure cancellation: its own subject)
    return _make_case(M, C, "none", x, dy, g)


@pytest.mark.parametrize("mean", [4.0, 30.0])
def test_bn_one_pass_variance_conditioning(backend, mean):
    """The statistics are one pass: var = E[x^2] - mean^2 from fp32 partial rows, so save_invstd loses about (mean / std)^2 fp32 rounding
    units.  Activations at mean 4, std 0.3 (the input of tests/test_kernels.py::test_bn_backward_input_gradient_sums_to_zero) hold the
    project's bars in every quantity.  At mean 30, std 0.3 save_invstd is asserted against the derived bound 2^-24 * (1 + (mean / std)^2) -
    one fp32 rounding unit of E[x^2] relative to the variance; the other quantities, and fp32 ATen (two passes) beside every figure, are
    printed."""
    _assert_geometry(BY_SHAPE[(2100, 8)])
    cs = _conditioning_case(mean)
    cs.bar = dict(QUANTITIES)
    if mean == 4.0:
        _chain(cs, backend, "contiguous")
        return
    cs.bar["save_invstd"] = 2.0 ** -24 * (1 + (mean / 0.3) ** 2)
    r = _chain(cs, backend, "contiguous", quantities=("sum", "sumsq", "save_mean", "save_invstd"))
    assert r.err["save_invstd"] <= cs.bar["save_invstd"]


# --------------------------------------------------------------------------------------------- 7. refusals
# Float offsets of the operands inside one NaN-filled buffer (M = 8, C = 8, ld = 8: matrices of 64 floats; 4200 partial rows of 4 channels),
# all 16-byte aligned and far from the buffer's end: were a check missing, the launch it lets through would still stay inside the buffer.
_AT = dict(x=0, dy=256, y=512, r1=768, r2=1024, dx=1280, g=1536, scale=1792, shift=1824, mean=1856, invstd=1888, gamma=1920, beta=1952, rm=1984, rv=2016,
           dgamma=2048, dbeta=2080, out=2112, a1=2144, coef=2176, parts=4096, sums=6144, ws=8192, big=16384)
_LD = dict(x_ld=8, dy_ld=8, y_ld=8, r1_ld=8, r2_ld=8, dx_ld=8, g_ld=8)


def test_bn_refusals(backend):
    """What the C side rejects, it rejects before any launch: a status, a message, and the NaN-filled buffer keeps its bits.  C % 4 != 0,
    M <= 0, a NULL operand, an activation code outside 0 .. 4, scale without shift, a workspace one byte short of what 4200 partial rows
    need with the fused switch off, and - the contract of include/sgx_hip.h - an address that is not a multiple of 16 bytes or a row stride
    that is not a multiple of 4 floats, in every operand the sweeps read or write as float4."""
    L, st = K.lib(), K.stream()
    buf = torch.full((65536,), NAN, device=backend)
    before = _bits(buf)
    base = K.ptr(buf)
    assert base % 16 == 0
    good = {k: base + 4 * v for k, v in _AT.items()}
    good.update(_LD, M=8, C=8, act=0)

    calls = {
        "channel_stats": lambda a: L.sgx_channel_stats_partial(a["x"], a["M"], a["C"], a["x_ld"], a["parts"], st),
        "affine_act": lambda a: L.sgx_affine_act_fwd(a["x"], a["x_ld"], a["scale"], a["shift"], a["r1"], a["r1_ld"], 1.0, a["a1"], a["r2"], a["r2_ld"], 1.0, a["y"],
                                                     a["y_ld"], a["M"], a["C"], a["act"], a["parts"], st),
        "bn_bwd_reduce": lambda a: L.sgx_bn_bwd_reduce(a["dy"], a["dy_ld"], a["x"], a["x_ld"], a["scale"], a["shift"], a["mean"], a["M"], a["C"], a["act"], a["parts"], st),
        "bn_bwd_apply": lambda a: L.sgx_bn_bwd_apply(a["dy"], a["dy_ld"], a["x"], a["x_ld"], a["scale"], a["shift"], a["coef"], a["dx"], a["dx_ld"], a["g"], a["g_ld"],
                                                     a["M"], a["C"], a["act"], st),
        "relu_bwd": lambda a: L.sgx_relu_bwd(a["dy"], a["dy_ld"], a["y"], a["y_ld"], a["g"], a["g_ld"], a["M"], a["C"], st),
        "relu_bwd_bn_reduce": lambda a: L.sgx_relu_bwd_bn_reduce(a["dy"], a["dy_ld"], a["y"], a["y_ld"], a["x"], a["x_ld"], a["mean"], a["g"], a["g_ld"], a["M"], a["C"],
                                                                 a["parts"], st),
        "axpy": lambda a: L.sgx_axpy(a["x"], a["x_ld"], 1.0, a["a1"], a["y"], a["y_ld"], a["M"], a["C"], 1, st),
        "dot": lambda a: L.sgx_dot(a["x"], a["x_ld"], a["y"], a["y_ld"], a["M"], a["C"], 1.0, a["out"], 0, a["ws"], 4096, st),
        "colsum": lambda a: L.sgx_colsum(a["x"], a["x_ld"], a["M"], a["C"], 4, 4 * a["x_ld"], a["out"], 0, a["ws"], st),
    }
    # the operands each entry point moves as float4 (pointers, then strides), and those it merely requires
    vec = {"channel_stats": (["x", "parts"], ["x_ld"]), "affine_act": (["x", "y", "r1", "r2", "scale", "shift", "parts"], ["x_ld", "y_ld", "r1_ld", "r2_ld"]),
           "bn_bwd_reduce": (["dy", "x", "scale", "shift", "mean", "parts"], ["dy_ld", "x_ld"]),
           "bn_bwd_apply": (["dy", "x", "scale", "shift", "coef", "dx", "g"], ["dy_ld", "x_ld", "dx_ld", "g_ld"]),
           "relu_bwd": (["dy", "y", "g"], ["dy_ld", "y_ld", "g_ld"]), "relu_bwd_bn_reduce": (["dy", "y", "x", "mean", "g", "parts"], ["dy_ld", "y_ld", "x_ld", "g_ld"]),
           "axpy": (["x", "y"], ["x_ld", "y_ld"]), "dot": (["x", "y"], ["x_ld", "y_ld"]), "colsum": (["x", "ws"], ["x_ld"])}
    required = {"channel_stats": ["x", "parts"], "affine_act": ["x", "y"], "bn_bwd_reduce": ["dy", "x", "scale", "shift", "mean", "parts"],
                "bn_bwd_apply": ["dy", "x", "scale", "shift", "coef", "dx"], "relu_bwd": ["dy", "y", "g"], "relu_bwd_bn_reduce": ["dy", "y", "x", "mean", "g", "parts"],
                "axpy": ["x", "y"], "dot": ["x", "y", "out", "ws"], "colsum": ["x", "out", "ws"]}

    def refused(rc, what, word, status=-1):
        msg = (L.sgx_last_error() or b"").decode()
        assert rc == status and word in msg, f"{what}: status {rc}, message {msg!r}"
        with pytest.raises(SgxError, match=what.split(":")[0]):
            K.check(rc, what)

    tried = 0
    for name, call in calls.items():
        for k, v in (("C", 6), ("C", 0), ("M", 0), ("M", -1)):
            refused(call({**good, k: v}), f"{name}: {k} = {v}", name)
            tried += 1
        for p in required[name]:
            refused(call({**good, p: None}), f"{name}: {p} = NULL", name)
            tried += 1
        pointers, strides = vec[name]
        for p, deltas in [(p, (4, 8)) for p in pointers] + [(s, (1, 2)) for s in strides]:
            for d in deltas:
                refused(call({**good, p: good[p] + d}), f"{name}: {p} off by {d}", "16 bytes")
                tried += 1
    assert tried == 9 * 4 + sum(map(len, required.values())) + 2 * sum(len(p) + len(s) for p, s in vec.values())
    for name in ("affine_act", "bn_bwd_reduce", "bn_bwd_apply"):
        for bad in (-1, 5):
            refused(calls[name]({**good, "act": bad}), f"{name}: activation {bad}", "activation")
    refused(calls["affine_act"]({**good, "shift": None}), "affine_act: scale without shift", "scale and shift")
    refused(calls["affine_act"]({**good, "scale": None}), "affine_act: shift without scale", "scale and shift")

    # finalizes: no partial rows / no rows; and 4200 partial rows of 4 channels with the switch off need 2 x 64 x 4 doubles of workspace
    a = SimpleNamespace(**good)
    nblk, C = 4200, 4
    need = 2 * 64 * C * 8
    assert L.sgx_reduce_workspace(nblk, C) == need + 256

    def finalize(nblk=nblk, wsb=need, ws=a.ws, parts=a.big, scale=a.scale):
        return L.sgx_bn_finalize(parts, nblk, 8400, C, a.gamma, a.beta, EPS, MOM, a.rm, a.rv, a.mean, a.invstd, scale, a.shift, ws, wsb, st)

    def bwd_finalize(nblk=nblk, wsb=need, ws=a.ws, parts=a.big, coef=a.coef):
        return L.sgx_bn_bwd_finalize(parts, nblk, 8400, C, a.gamma, a.mean, a.invstd, a.dgamma, a.dbeta, coef, ws, wsb, st)

    def reduce_sums(nblk=nblk, wsb=need, ws=a.ws, parts=a.big, sums=a.sums):
        return L.sgx_bn_reduce_sums(parts, nblk, C, sums, ws, wsb, st)

    refused(finalize(nblk=0), "bn_finalize: no partial rows", "bn_finalize")
    refused(finalize(parts=None), "bn_finalize: parts = NULL", "bn_finalize")
    refused(finalize(scale=None), "bn_finalize: scale = NULL", "bn_finalize")
    refused(bwd_finalize(parts=None), "bn_bwd_finalize: parts = NULL", "bn_bwd_finalize")
    refused(bwd_finalize(coef=None), "bn_bwd_finalize: coef = NULL", "bn_bwd_finalize")
    refused(reduce_sums(nblk=0), "bn_reduce_sums: no partial rows", "bn_reduce_sums")
    refused(reduce_sums(sums=None), "bn_reduce_sums: sums = NULL", "bn_reduce_sums")
    refused(L.sgx_bn_finalize_sums(a.sums, 0, C, a.gamma, a.beta, EPS, MOM, a.rm, a.rv, a.mean, a.invstd, a.scale, a.shift, st), "bn_finalize_sums: M = 0",
            "bn_finalize_sums")
    refused(L.sgx_bn_finalize_sums(None, 8, C, a.gamma, a.beta, EPS, MOM, a.rm, a.rv, a.mean, a.invstd, a.scale, a.shift, st), "bn_finalize_sums: sums = NULL",
            "bn_finalize_sums")
    refused(L.sgx_bn_bwd_finalize_sums(a.sums, a.sums, 0, C, a.gamma, a.mean, a.invstd, a.dgamma, a.dbeta, a.coef, st), "bn_bwd_finalize_sums: M = 0",
            "bn_bwd_finalize_sums")
    refused(L.sgx_bn_bwd_finalize_sums(None, a.sums, 8, C, a.gamma, a.mean, a.invstd, a.dgamma, a.dbeta, a.coef, st), "bn_bwd_finalize_sums: local = NULL",
            "bn_bwd_finalize_sums")
    prev = L.sgx_bn_get_fused_finalize()
    try:
        L.sgx_bn_set_fused_finalize(0)
        for name, call in (("bn_finalize", finalize), ("bn_bwd_finalize", bwd_finalize), ("bn_reduce_sums", reduce_sums)):
            refused(call(wsb=need - 1), f"{name}: workspace one byte short", "workspace", status=-4)
            refused(call(ws=None), f"{name}: no workspace", "workspace", status=-4)
    finally:
        L.sgx_bn_set_fused_finalize(prev)
    assert L.sgx_bn_get_fused_finalize() == 1
    assert torch.equal(_bits(buf), before), "a refused call wrote to its buffers"
