"""BEiT's glue kernels (csrc/vit.h: sgx_attn_rpb_fwd / _bwd, sgx_layerscale_fwd / _bwd, sgx_token_mean_fwd / _bwd, sgx_token_assemble_* without a
position embedding) against torch in fp64 on the CPU, on the chip and on the host emulation of the same sources.

Bars (the project's own, tests/test_vit_kernels.py): 2e-5 of the tensor's max-abs for element-wise results, 1e-4 for results that are sums over
rows (dtable, dgamma).  Every case runs with contiguous operands and with every operand a channel slice of a wider NaN-filled buffer: the
surroundings of every output keep their bits, no output element is NaN.  The attention reference is fp64 autograd with bias = table[index],
the index from this file's own closed form (and that closed form against the reference's recorded index, tests/golden/beit_index_reference.pt).
Every comparison prints `BEIT_ERR <kernel> <quantity> <bar> <measured>` before it asserts (pytest -rP shows the lines).
"""
import functools
import os

import pytest
import torch

from util import rel_err

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

from test_vit_kernels import LAYOUTS, NAN, TOL, TOL_SUM, _Watch, _base, _bits, _seed, _view

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beit_index_reference.pt")
# (B, heads, (gh, gw), d, q / k magnitude): the real geometry (T = 197: a 5-row tail in the fourth 64-row tile, N = 732); T = 65, one row past a
# workgroup tile, three images for the batch-order sum; T = 17, one row past a 16-row sub-tile; T = 16 on a non-square grid with the d > 64
# instantiation; T = 2, N = 4, three of whose four bins are the class token's.  Magnitudes as in test_vit_kernels.ATTN_FIXED.
ATTN_RPB = [(2, 3, (14, 14), 64, 1.0), (3, 2, (8, 8), 32, 4.0), (2, 4, (4, 4), 16, 6.0), (2, 1, (3, 5), 80, 2.0), (1, 2, (1, 1), 16, 1.0)]
TABLE_MAGS = (1.0, 6.0)


def _close(got, ref, tol, kernel, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"{kernel} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    e = rel_err(got, ref)
    print(f"BEIT_ERR {kernel} {what} {tol:g} {e:.3e}")
    assert e <= tol, f"{kernel} {what}: max err {e:.3e} of the tensor's max-abs > {tol}"


def closed_form_index(gh, gw):
    """index(i, j) over the tokens of a gh x gw grid behind one class token, written out pair by pair."""
    n = (2 * gh - 1) * (2 * gw - 1) + 3
    t = gh * gw + 1
    idx = torch.empty(t, t, dtype=torch.int64)
    for i in range(t):
        for j in range(t):
            if i == 0 and j == 0:
                idx[i, j] = n - 1
            elif i == 0:
                idx[i, j] = n - 3
            elif j == 0:
                idx[i, j] = n - 2
            else:
                (yi, xi), (yj, xj) = divmod(i - 1, gw), divmod(j - 1, gw)
                idx[i, j] = (yi - yj + gh - 1) * (2 * gw - 1) + (xi - xj + gw - 1)
    return idx


_index = functools.lru_cache(maxsize=None)(closed_form_index)


@pytest.mark.parametrize("grid", [s[2] for s in ATTN_RPB], ids=lambda g: f"{g[0]}x{g[1]}")
def test_closed_form_index_equals_the_reference(grid):
    """The recorded outputs of the reference's gen_relative_position_index for the five grids; every bin of every table is used."""
    recorded = torch.load(GOLDEN, weights_only=True)[f"{grid[0]}x{grid[1]}"]
    mine = _index(*grid)
    assert recorded.dtype == torch.int64 and torch.equal(mine, recorded)
    assert mine.unique().numel() == K.rpb_rows(grid), "a table row that no token pair uses"
    from super_gradients_amd.training.models.classification_models.beit import relative_position_index

    assert torch.equal(relative_position_index(grid), recorded), "the model's own closed form"


# --------------------------------------------------------------------------------------------- attention with the bias
@functools.lru_cache(maxsize=None)
def _case(B, H, grid, d, mag, tmag):
    """Inputs and the fp64 autograd reference, built once and shared by both back ends and both layouts."""
    T, N = grid[0] * grid[1] + 1, K.rpb_rows(grid)
    g = torch.Generator().manual_seed(_seed(B, H, T, d, int(mag * 10), int(tmag)))
    D = H * d
    qkv = torch.randn(B, T, 3 * D, generator=g)
    qkv[..., :2 * D] *= mag
    do = torch.randn(B, T, D, generator=g)
    table = torch.randn(N, H, generator=g) * tmag
    dt0 = torch.randn(N, H, generator=g)
    scale = d ** -0.5
    q, k, v = [t.double().reshape(B, T, H, d).permute(0, 2, 1, 3).clone().requires_grad_(True) for t in qkv.split(D, dim=-1)]
    tab = table.double().requires_grad_(True)
    bias = tab[_index(*grid).reshape(-1)].reshape(T, T, H).permute(2, 0, 1)
    s = (q @ k.transpose(-1, -2)) * scale + bias
    o = s.softmax(-1) @ v
    o.backward(do.double().reshape(B, T, H, d).permute(0, 2, 1, 3))
    back = lambda t: t.detach().permute(0, 2, 1, 3).reshape(B, T, 1, D)  # noqa: E731
    return dict(qkv=qkv, do=do, table=table, dt0=dt0, scale=scale, o=back(o), lse=torch.logsumexp(s.detach(), -1), dq=back(q.grad), dk=back(k.grad),
                dv=back(v.grad), dtable=tab.grad)


def _run(case, B, H, grid, d, dev, layout, table=None, dtable=None):
    T, D = grid[0] * grid[1] + 1, H * d
    table = case["table"].to(dev) if table is None else table
    dtable = case["dt0"].clone().to(dev) if dtable is None else dtable
    qkv = _view((B, T, 1, 3 * D), dev, layout, 0, case["qkv"])
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    o = _view((B, T, 1, D), dev, layout, 1)
    w = _Watch(o)
    _, lse = K.attn_rpb_fwd(q, k, v, H, case["scale"], table, grid, out=o)
    w.check("attn_rpb_fwd")
    do = _view((B, T, 1, D), dev, layout, 1, case["do"])
    dqkv = _view((B, T, 1, 3 * D), dev, layout, 3)
    w = _Watch(dqkv)
    K.attn_rpb_bwd(q, k, v, o, do, lse, H, case["scale"], table, grid, dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], dtable)
    w.check("attn_rpb_bwd")
    return qkv, o, lse, do, dqkv, dtable


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tmag", TABLE_MAGS, ids=lambda m: f"table{m:g}")
@pytest.mark.parametrize("shape", ATTN_RPB, ids=lambda s: f"{s[0]}x{s[1]}x{s[2][0]}x{s[2][1]}x{s[3]}")
def test_attention_with_bias(backend, shape, tmag, layout):
    B, H, grid, d, mag = shape
    T, D, N = grid[0] * grid[1] + 1, H * d, K.rpb_rows(grid)
    case = _case(B, H, grid, d, mag, tmag)
    dev = backend
    qkv, o, lse, do, dqkv, dtable = _run(case, B, H, grid, d, dev, layout)
    tag = f"attn_rpb[{B},{H},{grid},{d},x{mag:g},table x{tmag:g},{layout}]"
    _close(o, case["o"], TOL, tag, "o")
    _close(lse, case["lse"], TOL, tag, "lse")
    for i, name in enumerate(("dq", "dk", "dv")):
        _close(dqkv[..., i * D:(i + 1) * D], case[name], TOL, tag, name)
    _close(dtable.cpu().double() - case["dt0"].double(), case["dtable"], TOL_SUM, tag, "dtable (added onto a non-zero view)")
    # twice: the same bits everywhere
    again = _run(case, B, H, grid, d, dev, layout)
    for a, b, name in zip((o, lse, dqkv, dtable), (again[1], again[2], again[4], again[5]), ("o", "lse", "dq / dk / dv", "dtable")):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {name} does not repeat its bits"
    # head h of the multi-head call == the one-head call on that head's slices and its table column (a strided [N, 1] view), bit for bit
    if H > 1:
        table = case["table"].to(dev)
        for h in range(H):
            sl = lambda t, part=0: t[..., part * D + h * d: part * D + (h + 1) * d]  # noqa: E731
            o1, lse1 = K.attn_rpb_fwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), 1, case["scale"], table[:, h:h + 1], grid)
            assert torch.equal(_bits(o1), _bits(sl(o))) and torch.equal(_bits(lse1[:, 0]), _bits(lse[:, h])), f"{tag}: head {h} forward differs from the one-head call"
            g1 = torch.full((B, T, 1, 3 * d), NAN, device=dev)
            dt1 = case["dt0"].clone().to(dev)
            K.attn_rpb_bwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), sl(o), sl(do), lse[:, h:h + 1].contiguous(), 1, case["scale"], table[:, h:h + 1], grid, g1[..., :d],
                           g1[..., d:2 * d], g1[..., 2 * d:], dt1[:, h:h + 1])
            for part in range(3):
                assert torch.equal(_bits(g1[..., part * d:(part + 1) * d]), _bits(sl(dqkv, part))), f"{tag}: head {h} backward part {part} differs from the one-head call"
            assert torch.equal(_bits(dt1[:, h]), _bits(dtable[:, h])), f"{tag}: head {h} table gradient differs from the one-head call"
            other = [c for c in range(H) if c != h]
            assert torch.equal(_bits(dt1[:, other]), _bits(case["dt0"][:, other])), f"{tag}: the one-head call wrote another head's table column"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ATTN_RPB, ids=lambda s: f"{s[0]}x{s[1]}x{s[2][0]}x{s[2][1]}x{s[3]}")
def test_zero_table_gives_the_plain_kernels_bits(backend, shape, layout):
    B, H, grid, d, mag = shape
    T, D, N = grid[0] * grid[1] + 1, H * d, K.rpb_rows(grid)
    case = _case(B, H, grid, d, mag, TABLE_MAGS[0])
    dev = backend
    qkv, o, lse, do, dqkv, _ = _run(case, B, H, grid, d, dev, layout, table=torch.zeros(N, H, device=dev))
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    o0 = _view((B, T, 1, D), dev, layout, 1)
    _, lse0 = K.attn_fwd(q, k, v, H, case["scale"], out=o0)
    g0 = _view((B, T, 1, 3 * D), dev, layout, 3)
    K.attn_bwd(q, k, v, o0, do, lse0, H, case["scale"], g0[..., :D], g0[..., D:2 * D], g0[..., 2 * D:])
    for a, b, name in ((o, o0, "o"), (lse, lse0, "lse"), (dqkv, g0, "dq / dk / dv")):
        assert torch.equal(_bits(a), _bits(b)), f"attn_rpb[{shape},{layout}] with a zero table: {name} differs from the plain kernel"


def _refused(call, *outs):
    before = [_bits(_base(o)) for o in outs]
    with pytest.raises(_lib.SgxError):
        call()
    for o, b in zip(outs, before):
        assert torch.equal(_bits(_base(o)), b), "a refused call wrote its output"


def test_attention_with_bias_refusals(backend):
    dev = backend
    full = lambda *s: torch.full(s, NAN, device=dev)  # noqa: E731
    lib = K.lib()
    cap = lib.sgx_attn_rpb_max_rows()
    assert cap == 4096, "ATT_RPB_MAXN changed: the header, DESIGN.md 20 and the grids here follow it"

    def calls(B, H, T, d, gh, gw, n_rows, tab_ld=None):
        """The C entry points themselves (the Python wrapper derives T and the table's shape and could not express these)."""
        D = H * d
        tab_ld = H if tab_ld is None else tab_ld
        qkv, o, lse, g = torch.zeros(B, T, 1, 3 * D, device=dev), full(B, T, 1, D), full(B, H, T), full(B, T, 1, 3 * D)
        table, dtable = torch.zeros(n_rows, max(tab_ld, H), device=dev), full(n_rows, max(tab_ld, H))
        p = K.ptr
        ws = torch.zeros(max(int(lib.sgx_attn_rpb_bwd_workspace(B, H, T, gh, gw)), 256), dtype=torch.uint8, device=dev)
        fwd = lambda: K.check(lib.sgx_attn_rpb_fwd(B, H, T, d, gh, gw, p(qkv), p(qkv[..., D:]), p(qkv[..., 2 * D:]), 3 * D, T * 3 * D, 1.0, p(table), tab_ld,  # noqa: E731
                                                   p(o), D, T * D, p(lse), K.stream()), "sgx_attn_rpb_fwd")
        bwd = lambda: K.check(lib.sgx_attn_rpb_bwd(B, H, T, d, gh, gw, p(qkv), p(qkv[..., D:]), p(qkv[..., 2 * D:]), 3 * D, T * 3 * D, p(o), p(o), D, T * D,  # noqa: E731
                                                   p(lse), 1.0, p(table), tab_ld, p(g), p(g[..., D:]), p(g[..., 2 * D:]), 3 * D, T * 3 * D, p(dtable), tab_ld,
                                                   p(ws), ws.numel(), K.stream()), "sgx_attn_rpb_bwd")
        _refused(fwd, o, lse)
        _refused(bwd, g, dtable)

    calls(1, 2, 18, 16, 4, 4, 52)               # T != gh * gw + 1
    calls(1, 1, 17, 132, 4, 4, 52)              # d > 128
    calls(1, 1, 33 * 33 + 1, 16, 33, 33, 4228)  # N = 65 * 65 + 3 = 4228 > the LDS cap
    calls(1, 4, 17, 16, 4, 4, 52, tab_ld=3)     # a table row stride below the head count: rows would overlap
    # the wrapper: a table whose heads are not contiguous, a table of another grid
    qkv, o = torch.zeros(1, 17, 1, 96, device=dev), full(1, 17, 1, 32)
    _refused(lambda: K.attn_rpb_fwd(qkv[..., :32], qkv[..., 32:64], qkv[..., 64:], 2, 1.0, torch.zeros(2, 52, device=dev).t(), (4, 4), out=o), o)
    _refused(lambda: K.attn_rpb_fwd(qkv[..., :32], qkv[..., 32:64], qkv[..., 64:], 2, 1.0, torch.zeros(28, 2, device=dev), (4, 4), out=o), o)
    # a misaligned operand, as the plain kernels refuse it
    wide = torch.zeros(1, 17, 1, 100, device=dev)
    _refused(lambda: K.attn_rpb_fwd(wide[..., 1:33], wide[..., 33:65], wide[..., 65:97], 2, 1.0, torch.zeros(52, 2, device=dev), (4, 4), out=o), o)


def test_largest_grid_under_the_cap(backend):
    """32 x 32 (N = 3972 of the 4096 the LDS budget allows): every thread of the dq pass owns 16 bins.  One image, one head, d = 4."""
    grid, d = (32, 32), 4
    T, N = 1025, K.rpb_rows((32, 32))
    assert N == 3972 <= K.lib().sgx_attn_rpb_max_rows()
    g = torch.Generator().manual_seed(11)
    qkv, do, table = torch.randn(1, T, 3 * d, generator=g), torch.randn(1, T, d, generator=g), torch.randn(N, 1, generator=g)
    q, k, v = [t.double().reshape(1, T, 1, d).permute(0, 2, 1, 3).clone().requires_grad_(True) for t in qkv.split(d, dim=-1)]
    tab = table.double().requires_grad_(True)
    # the index of a square grid without the T x T Python loop: the same closed form, vectorised
    t = torch.arange(T - 1)
    y, x = t // 32, t % 32
    idx = torch.empty(T, T, dtype=torch.int64)
    idx[1:, 1:] = (y[:, None] - y[None, :] + 31) * 63 + (x[:, None] - x[None, :] + 31)
    idx[0, :], idx[:, 0], idx[0, 0] = N - 3, N - 2, N - 1
    s = (q @ k.transpose(-1, -2)) * 0.5 + tab[idx.reshape(-1)].reshape(T, T, 1).permute(2, 0, 1)
    o = s.softmax(-1) @ v
    o.backward(do.double().reshape(1, T, 1, d).permute(0, 2, 1, 3))
    dev = backend
    qd = qkv.reshape(1, T, 1, 3 * d).to(dev)
    og, lse = K.attn_rpb_fwd(qd[..., :d], qd[..., d:2 * d], qd[..., 2 * d:], 1, 0.5, table.to(dev), grid)
    gq, dt = torch.full((1, T, 1, 3 * d), NAN, device=dev), torch.zeros(N, 1, device=dev)
    K.attn_rpb_bwd(qd[..., :d], qd[..., d:2 * d], qd[..., 2 * d:], og, do.reshape(1, T, 1, d).to(dev), lse, 1, 0.5, table.to(dev), grid, gq[..., :d], gq[..., d:2 * d],
                   gq[..., 2 * d:], dt)
    back = lambda a: a.detach().permute(0, 2, 1, 3).reshape(1, T, 1, d)  # noqa: E731
    _close(og, back(o), TOL, "attn_rpb[32x32]", "o")
    _close(gq[..., :d], back(q.grad), TOL, "attn_rpb[32x32]", "dq")
    _close(gq[..., d:2 * d], back(k.grad), TOL, "attn_rpb[32x32]", "dk")
    _close(dt, tab.grad, TOL_SUM, "attn_rpb[32x32]", "dtable")


# --------------------------------------------------------------------------------------------- layer scale
LS_SHAPES = [(2, 17, 64), (1, 197, 192), (3, 5, 4)]  # (images, rows per image, C); 15 rows: not a multiple of the sweep's block rows


@functools.lru_cache(maxsize=None)
def _ls_case(B, T, C):
    g = torch.Generator().manual_seed(_seed(B, T, C, "ls"))
    x, t, dy = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    gamma, dg0 = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g)
    keep = torch.zeros(B)
    keep[::2] = 1.0  # (one image: kept; otherwise at least one kept and one dropped)
    m = keep * 2.0 if B > 1 else torch.full((1,), 2.0)  # 0 or 1 / keep with keep = 0.5
    return dict(x=x, t=t, dy=dy, gamma=gamma, dg0=dg0, m=m)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("with_m", [False, True], ids=["no-m", "m"])
@pytest.mark.parametrize("with_gamma", [False, True], ids=["no-gamma", "gamma"])
@pytest.mark.parametrize("shape", LS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_scale(backend, shape, with_gamma, with_m, layout):
    B, T, C = shape
    case = _ls_case(B, T, C)
    dev = backend
    assert K.lib().sgx_layerscale_bwd_workspace(B * T, C) == -(-B * T // K.lib().sgx_layerscale_block_rows()) * C * 4 + 256
    if B > 1:
        assert bool((case["m"] == 0).any()) and bool((case["m"] == 2.0).any())
    tag = f"layerscale[{shape},{'gamma' if with_gamma else '-'},{'m' if with_m else '-'},{layout}]"
    shp = (B, T, 1, C)
    gamma, m = (case["gamma"].to(dev) if with_gamma else None), (case["m"].to(dev) if with_m else None)
    x64, t64, g64 = case["x"].double(), case["t"].double().requires_grad_(True), case["gamma"].double().requires_grad_(True)
    m64 = case["m"].double().view(B, 1, 1) if with_m else 1.0
    y64 = x64 + m64 * ((g64 if with_gamma else 1.0) * t64)
    y64.backward(case["dy"].double())
    x, t = _view(shp, dev, layout, 0, case["x"]), _view(shp, dev, layout, 1, case["t"])
    y = _view(shp, dev, layout, 2)
    w = _Watch(y)
    K.layerscale_fwd(x, t, gamma, m, out=y)
    w.check(tag)
    _close(y, y64.reshape(shp), TOL, tag, "y")
    xin = _view(shp, dev, layout, 0, case["x"])
    K.layerscale_fwd(xin, t, gamma, m, out=xin)
    assert torch.equal(_bits(xin), _bits(y)), f"{tag}: the in-place forward differs"
    dy = _view(shp, dev, layout, 3, case["dy"])
    results = []
    for rep in range(2):
        dt = _view(shp, dev, layout, 4)
        dgamma = case["dg0"].clone().to(dev) if with_gamma else None
        w = _Watch(dt)
        K.layerscale_bwd(dy, t, gamma, m, dgamma, out=dt)
        w.check(tag)
        results.append((dt, dgamma))
    dt, dgamma = results[0]
    _close(dt, t64.grad.reshape(shp), TOL, tag, "dt")
    assert torch.equal(_bits(dt), _bits(results[1][0])), f"{tag}: dt does not repeat its bits"
    if with_gamma:
        _close(dgamma.cpu().double() - case["dg0"].double(), g64.grad, TOL_SUM, tag, "dgamma (added onto a non-zero view)")
        assert torch.equal(_bits(dgamma), _bits(results[1][1])), f"{tag}: dgamma does not repeat its bits"
    inplace = _view(shp, dev, layout, 3, case["dy"])
    K.layerscale_bwd(inplace, t, gamma, m, case["dg0"].clone().to(dev) if with_gamma else None, out=inplace)
    assert torch.equal(_bits(inplace), _bits(dt)), f"{tag}: the in-place backward differs"


def test_layer_scale_refusals(backend):
    dev = backend
    x, y = torch.zeros(2, 3, 1, 10, device=dev), torch.full((2, 3, 1, 8), NAN, device=dev)
    _refused(lambda: K.layerscale_fwd(x[..., :8], x[..., :8], None, None, out=y), y)          # a row stride that is not a multiple of 4
    x = torch.zeros(2, 3, 1, 12, device=dev)
    _refused(lambda: K.layerscale_fwd(x[..., 1:9], x[..., 1:9], None, None, out=y), y)        # a misaligned address
    _refused(lambda: K.layerscale_bwd(x[..., :8], None, None, None, torch.zeros(8, device=dev), out=y), y)  # dgamma without gamma and t


# --------------------------------------------------------------------------------------------- patch-token mean, token assembly without pos
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 17, 64), (2, 197, 192)], ids=lambda s: "x".join(map(str, s)))
def test_token_mean(backend, shape, layout):
    B, T, D = shape
    dev = backend
    g = torch.Generator().manual_seed(_seed(B, T, D, "mean"))
    x, dy = torch.randn(B, T, D, generator=g) + 0.3, torch.randn(B, D, generator=g)
    x64 = x.double().requires_grad_(True)
    y64 = x64[:, 1:].mean(dim=1)
    y64.backward(dy.double())
    tag = f"token_mean[{shape},{layout}]"
    xv = _view((B, T, 1, D), dev, layout, 0, x)
    y = _view((B, 1, 1, D), dev, layout, 1)
    w = _Watch(y)
    K.token_mean_fwd(xv, out=y)
    w.check(tag)
    _close(y, y64.reshape(B, 1, 1, D), TOL, tag, "y")
    dx = _view((B, T, 1, D), dev, layout, 2)
    w = _Watch(dx)
    K.token_mean_bwd(_view((B, 1, 1, D), dev, layout, 3, dy), T, out=dx)
    w.check(tag)
    _close(dx, x64.grad.reshape(B, T, 1, D), TOL, tag, "dx")
    assert not bool(dx[:, 0].any()), f"{tag}: the class-token row of the gradient is not exactly zero"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_token_assembly_without_a_position_embedding(backend, layout):
    B, T, D = 3, 17, 12
    dev = backend
    g = torch.Generator().manual_seed(_seed(B, T, "nopos"))
    patch, cls = torch.randn(B, T - 1, D, generator=g), torch.randn(1, 1, D, generator=g)
    patch[0, 0, 0] = -0.0  # (moved, not added to a zero)
    out = _view((B, T, 1, D), dev, layout, 1)
    w = _Watch(out)
    K.token_assemble_fwd(_view((B, T - 1, 1, D), dev, layout, 0, patch), cls.to(dev), None, out=out)
    w.check("token_assemble_fwd")
    assert torch.equal(_bits(out), _bits(torch.cat((cls.expand(B, 1, D), patch), dim=1).reshape(B, T, 1, D))), "token assembly without pos differs from cat"
    dx, dcls0 = torch.randn(B, T, D, generator=g), torch.randn(1, 1, D, generator=g)
    dcls = dcls0.clone().to(dev)
    K.token_assemble_bwd(_view((B, T, 1, D), dev, layout, 2, dx), dcls, None)
    _close(dcls.cpu().double() - dcls0.double(), dx.double().sum(0, keepdim=True)[:, :1], TOL_SUM, f"token_assemble_bwd[no pos,{layout}]", "dcls (added)")
