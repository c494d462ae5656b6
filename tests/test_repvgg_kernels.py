"""The RepVGG branch-sum sweeps (csrc/bn.hip: sgx_tri_affine_act_fwd, sgx_tri_affine_act_bwd_reduce) against plain torch, with fewer than three
branches (a null branch is a branch of zero scale and shift, bit for bit), and across launch geometries."""
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, empty_nhwc, to_nchw_cpu, to_nhwc

from super_gradients_amd import kernels as K

TOL = 2e-5  # (tests/test_kernels.py's bar for element-wise sweeps)
ACTS = {"relu": F.relu, "silu": F.silu, None: lambda t: t}


def _shape(backend, c):
    """RepVggA0's stage widths; rows: several row blocks on the chip, a few rows of one block on the emulation.  c = 4: one channel group,
    256 row lanes, most of them idle; c = 260: 65 channel groups = two channel strips, the second with one live group."""
    if c == 4:
        return (1, 3, 5, 4)
    if backend.type == "cuda":
        return (3, 23, 19, c) if c < 1000 else (2, 7, 7, c)
    return (2, 5, 3, c) if c < 1000 else (1, 3, 2, c)


def _case(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    t3, t1, x, r, dy = (torch.randn(n, c, h, w, generator=g) for _ in range(5))
    vec = lambda lo, hi: torch.rand(c, generator=g) * (hi - lo) + lo  # noqa: E731
    sb = [(vec(0.5, 1.5), vec(-0.3, 0.3)) for _ in range(3)]
    means = [vec(-0.2, 0.2) for _ in range(3)]
    return (t3, t1, x, r, dy), sb, means


def _bc(v):
    return v.view(1, -1, 1, 1)


def _finalized(parts, M, backend):
    """mean / biased variance out of bn_finalize - the consumer of the rows in the blocks."""
    c = parts.shape[2]
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    eps = 1e-5
    _, _, mean, invstd = K.bn_finalize(parts, M, one, zero, eps, 0.1, zero.clone(), one.clone())
    return mean.cpu().double(), 1.0 / invstd.cpu().double() ** 2 - eps


@pytest.mark.parametrize("c", [4, 48, 96, 260, 1280])
@pytest.mark.parametrize("act", ["relu", "silu", None])
@pytest.mark.parametrize("post_add,stats", [(False, False), (True, True), (False, True), (True, False)])
def test_tri_affine_act_forward(backend, c, act, post_add, stats):
    """y = act(s3 t3 + b3 + s1 t1 + b1 + sI x + bI) [+ r] on strided operands, with and without the statistics rows of the stored value."""
    n, h, w, _ = _shape(backend, c)
    (t3, t1, x, r, _), sb, _ = _case(n, h, w, c, 3)
    pre = sum(_bc(s).double() * t.double() + _bc(b).double() for t, (s, b) in zip((t3, t1, x), sb))
    ref = ACTS[act](pre) + (r.double() if post_add else 0.0)
    d = lambda v: v.to(backend)  # noqa: E731
    out = empty_nhwc(n, h, w, c, backend, ld_pix=c + 8, c_off=4)
    res = K.tri_affine_act(to_nhwc(t3, backend, ld_pix=c + 4), d(sb[0][0]), d(sb[0][1]), to_nhwc(t1, backend), d(sb[1][0]), d(sb[1][1]),
                           to_nhwc(x, backend, ld_pix=c + 12, c_off=8), d(sb[2][0]), d(sb[2][1]), post_add=to_nhwc(r, backend) if post_add else None,
                           act=act, out=out, want_stats=stats)
    y = res[0] if stats else res
    assert y.data_ptr() == out.data_ptr()
    assert_close(to_nchw_cpu(y), ref.float(), TOL, f"tri_affine_act {act}")
    if stats:
        parts = res[1]
        M = n * h * w
        assert tuple(parts.shape) == (2, K.stats_blocks(M), c)
        stored = to_nchw_cpu(y).double()
        mean, var = _finalized(parts, M, backend)
        assert_close(mean, stored.mean((0, 2, 3)), 1e-4, "mean of the stored y")
        assert_close(var, stored.var((0, 2, 3), unbiased=False), 1e-4, "variance of the stored y")
        assert_close(parts[0].sum(0).cpu(), stored.sum((0, 2, 3)).float(), 1e-4, "sum y")


@pytest.mark.parametrize("c", [4, 48, 96, 260, 1280])
@pytest.mark.parametrize("act", ["relu", "silu", None])
def test_tri_affine_act_bwd_reduce(backend, c, act):
    """g = dy act'(pre) and the reduce rows of the three BatchNorm backward passes: against autograd in fp64, and against bn_bwd's own
    reduce sweep over the stored g."""
    n, h, w, _ = _shape(backend, c)
    (t3, t1, x, _, dy), sb, means = _case(n, h, w, c, 4)
    pre = sum(_bc(s).double() * t.double() + _bc(b).double() for t, (s, b) in zip((t3, t1, x), sb)).requires_grad_(True)
    (gref,) = torch.autograd.grad(ACTS[act](pre), pre, dy.double())
    d = lambda v: v.to(backend)  # noqa: E731
    ops = (to_nhwc(t3, backend, ld_pix=c + 4), to_nhwc(t1, backend), to_nhwc(x, backend, ld_pix=c + 12, c_off=8))
    out = empty_nhwc(n, h, w, c, backend, ld_pix=c + 8, c_off=4)
    g, p3, p1, pi = K.tri_affine_act_bwd_reduce(to_nhwc(dy, backend, ld_pix=c + 4), ops[0], d(sb[0][0]), d(sb[0][1]), d(means[0]), ops[1], d(sb[1][0]),
                                                d(sb[1][1]), d(means[1]), ops[2], d(sb[2][0]), d(sb[2][1]), d(means[2]), act=act, out=out)
    assert_close(to_nchw_cpu(g), gref.float(), TOL, f"g {act}")
    gs = to_nchw_cpu(g).double()  # the sums are those of the g values that were stored
    M = n * h * w
    for name, parts, t, mu in (("3x3", p3, t3, means[0]), ("1x1", p1, t1, means[1]), ("identity", pi, x, means[2])):
        assert tuple(parts.shape) == (2, K.stats_blocks(M), c)
        assert_close(parts[0].sum(0).cpu(), gs.sum((0, 2, 3)).float(), 1e-4, f"sum g ({name})")
        assert_close(parts[1].sum(0).cpu(), (gs * (t.double() - _bc(mu).double())).sum((0, 2, 3)).float(), 1e-4, f"sum g (x - mean) ({name})")
    # each pair is what the BatchNorm backward's own reduce sweep leaves for (g, operand): bn_bwd(parts=...) gives the same dx / dgamma / dbeta
    gam, inv = torch.rand(c) + 0.5, torch.rand(c) + 0.5
    for parts, t, (s, b), mu in ((p3, ops[0], sb[0], means[0]), (pi, ops[2], sb[2], means[2])):
        dg0, db0, dg1, db1 = (torch.zeros(c, device=backend) for _ in range(4))
        dx0 = K.bn_bwd(g, t, d(s), d(b), d(gam), d(mu), d(inv), dg0, db0, act=None)
        dx1 = K.bn_bwd(g, t, d(s), d(b), d(gam), d(mu), d(inv), dg1, db1, act=None, parts=parts)
        assert torch.equal(dx0.cpu(), dx1.cpu()) and torch.equal(dg0.cpu(), dg1.cpu()) and torch.equal(db0.cpu(), db1.cpu())


@pytest.mark.parametrize("act", ["relu", "silu", None])
@pytest.mark.parametrize("post_add", [False, True])
def test_null_third_branch_is_the_two_branch_sweep(backend, act, post_add):
    """A null branch is a branch with zero scale and shift, bit for bit (adding +0.0 is exact, and this data has no -0.0 pre-activation): for
    y, for g and for the reduce rows of the branches that remain - without the third operand and without the second.  The statistics output
    does not change what is stored either."""
    n, h, w, c = _shape(backend, 96)
    (t3, t1, x, r, dy), sb, means = _case(n, h, w, c, 5)
    d = lambda v: v.to(backend)  # noqa: E731
    a, b, e = to_nhwc(t3, backend, ld_pix=c + 4), to_nhwc(t1, backend), to_nhwc(x, backend, ld_pix=c + 12, c_off=8)
    zero = torch.zeros(c, device=backend)
    rr = to_nhwc(r, backend) if post_add else None
    one, two = (a, d(sb[0][0]), d(sb[0][1])), (a, d(sb[0][0]), d(sb[0][1]), b, d(sb[1][0]), d(sb[1][1]))
    y2 = K.tri_affine_act(*two, post_add=rr, act=act)
    y2s, parts = K.tri_affine_act(*two, post_add=rr, act=act, want_stats=True)
    assert torch.equal(y2.cpu(), y2s.cpu())
    assert_close(parts[0].sum(0).cpu(), y2.cpu().double().sum((0, 1, 2)).float(), 1e-4, "sum y")
    y3, parts3 = K.tri_affine_act(*two, e, zero, zero, post_add=rr, act=act, want_stats=True)
    assert torch.equal(y2.cpu(), y3.cpu()) and torch.equal(parts.cpu(), parts3.cpu())
    assert torch.equal(y2.cpu(), K.tri_affine_act(*two, e, zero, zero, post_add=rr, act=act).cpu())
    y1 = K.tri_affine_act(*one, post_add=rr, act=act)
    assert torch.equal(y1.cpu(), K.tri_affine_act(*one, b, zero, zero, post_add=rr, act=act).cpu())
    dyd = to_nhwc(dy, backend)
    m = [d(v) for v in means]
    one, two = one + (m[0],), two[:3] + (m[0],) + two[3:] + (m[1],)
    g2, p3, p1, pi = K.tri_affine_act_bwd_reduce(dyd, *two, act=act)
    assert pi is None
    g3, q3, q1, qi = K.tri_affine_act_bwd_reduce(dyd, *two, e, zero, zero, m[2], act=act)
    assert qi is not None
    assert torch.equal(g2.cpu(), g3.cpu()) and torch.equal(q3.cpu(), p3.cpu()) and torch.equal(q1.cpu(), p1.cpu())
    g1, r3, r1, ri = K.tri_affine_act_bwd_reduce(dyd, *one, act=act)
    assert r1 is None and ri is None
    g1z, z3, z1, zi = K.tri_affine_act_bwd_reduce(dyd, *one, b, zero, zero, m[1], act=act)
    assert zi is None and z1 is not None
    assert torch.equal(g1.cpu(), g1z.cpu()) and torch.equal(r3.cpu(), z3.cpu())


@pytest.mark.parametrize("c", [4, 48, 260, 1280])
def test_launch_geometry_does_not_change_the_result(backend, c):
    """Three row-block counts: the stored y / g are the same bits (a lane's arithmetic does not depend on the grid), and a repeated launch on
    one geometry repeats its partial rows exactly (fixed order, no atomics).  The partial rows are one per row block, so their count follows the
    geometry; what the finalize makes of them - the fp64 column sums - may differ between geometries only by fp32 round-off, bounded from the
    number formats (no measured figure): a lane adds its L = ceil(rows_per_block / row_lanes) terms in fp32 (each term a rounded product:
    at most (L + 1) * 2^-24 relative to the sum of the terms' magnitudes), the lanes meet in fp64 and the row is rounded once to fp32
    (2^-24 more): per side (L + 2) * 2^-24 * sum |terms|."""
    n, h, w, _ = _shape(backend, c)
    (t3, t1, x, r, dy), sb, means = _case(n, h, w, c, 6)
    d = lambda v: v.to(backend)  # noqa: E731
    M = n * h * w
    ops = [to_nhwc(t, backend) for t in (t3, t1, x)]
    args = (ops[0], d(sb[0][0]), d(sb[0][1]), ops[1], d(sb[1][0]), d(sb[1][1]), ops[2], d(sb[2][0]), d(sb[2][1]))
    geoms = (None, 3, M)  # the default, a few long row blocks, one row per block

    def terms_per_lane(blocks):
        nblk = K.stats_blocks(M) if blocks is None else blocks
        row_lanes = 256 // min(c // 4, 64)
        return -(-(-(-M // nblk)) // row_lanes)

    def same_sums(pa, ba, pb, bb, mag, what):
        """pa / pb: [blocks, C] rows of two geometries; mag: [C] sum of the terms' magnitudes (fp64, from the stored tensors)."""
        bound = (terms_per_lane(ba) + terms_per_lane(bb) + 4) * 2.0 ** -24 * mag
        diff = (pa.cpu().double().sum(0) - pb.cpu().double().sum(0)).abs()
        assert bool((diff <= bound).all()), f"{what}: column sums differ by {float((diff / bound).max()):.2f} x the fp32 round-off bound"

    fwd = [K.tri_affine_act(*args, post_add=to_nhwc(r, backend), act="relu", want_stats=True, blocks=b) for b in geoms]
    again = K.tri_affine_act(*args, post_add=to_nhwc(r, backend), act="relu", want_stats=True, blocks=3)
    assert torch.equal(again[0].cpu(), fwd[1][0].cpu()) and torch.equal(again[1].cpu(), fwd[1][1].cpu())
    for (y, parts), b in zip(fwd[1:], geoms[1:]):
        assert parts.shape[1] == b
        assert torch.equal(y.cpu(), fwd[0][0].cpu()), f"y differs with {b} row blocks"
        ys = y.cpu().double()
        same_sums(parts[0], b, fwd[0][1][0], None, ys.abs().sum((0, 1, 2)), f"sum y, {b} row blocks")
        same_sums(parts[1], b, fwd[0][1][1], None, (ys * ys).sum((0, 1, 2)), f"sum y^2, {b} row blocks")
    margs = (to_nhwc(dy, backend), ops[0], d(sb[0][0]), d(sb[0][1]), d(means[0]), ops[1], d(sb[1][0]), d(sb[1][1]), d(means[1]), ops[2], d(sb[2][0]),
             d(sb[2][1]), d(means[2]))
    bwd = [K.tri_affine_act_bwd_reduce(*margs, act="relu", blocks=b) for b in geoms]
    again = K.tri_affine_act_bwd_reduce(*margs, act="relu", blocks=3)
    assert all(torch.equal(u.cpu(), v.cpu()) for u, v in zip(again, bwd[1]))
    for res, b in zip(bwd[1:], geoms[1:]):
        assert torch.equal(res[0].cpu(), bwd[0][0].cpu()), f"g differs with {b} row blocks"
        gs = res[0].cpu().double()
        for k, t, mu in ((1, t3, means[0]), (2, t1, means[1]), (3, x, means[2])):
            assert res[k].shape[1] == b
            centred = t.permute(0, 2, 3, 1).double() - mu.double()
            same_sums(res[k][0], b, bwd[0][k][0], None, gs.abs().sum((0, 1, 2)), f"sum g of pair {k}, {b} row blocks")
            same_sums(res[k][1], b, bwd[0][k][1], None, (gs * centred).abs().sum((0, 1, 2)), f"sum g (x - mean) of pair {k}, {b} row blocks")
