"""Hard-swish in the sweeps and depthwise epilogues, the BatchNorm -> SE gate -> activation sweeps (csrc/se.hip: sgx_bn_gate_act_fwd /
_bwd_gate / _bwd_data) and dropout (csrc/bn.hip: sgx_dropout_fwd), against plain torch in fp64 and autograd - on the chip and on the host
emulation of the same sources."""
import math

import pytest
import torch
import torch.nn.functional as F

from util import assert_close, to_nchw_cpu, to_nhwc

from super_gradients_amd import _lib
from super_gradients_amd import kernels as K

TOL = 2e-5  # (tests/test_kernels.py's bar for element-wise sweeps)


def hswish(t):
    return t * F.relu6(t + 3.0) / 6.0  # the reference's h_swish (classification_models/mobilenetv3.py:34-49)


# --------------------------------------------------------------------------------------------- hard-swish
def _hswish_inputs(backend):
    """Pre-activations on both sides of -3 and 3 that include exactly -3.0 and 3.0 (scale 1, shift 0: the pre-activation is the input, exactly)."""
    n, h, w, c = (2, 9, 7, 32) if backend.type == "cuda" else (1, 3, 2, 16)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, c, h, w, generator=g) * 3.0
    flat = x.view(-1)
    flat[0::7] = -3.0
    flat[3::7] = 3.0
    return x, torch.randn(n, c, h, w, generator=g), c


def test_hswish_affine_act_forward(backend):
    x, _, c = _hswish_inputs(backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    ref = hswish(x.double())
    for y in (K.affine_act(to_nhwc(x, backend), one, zero, act="hswish"), K.affine_act(to_nhwc(x, backend), act="hswish")):
        got = to_nchw_cpu(y)
        assert_close(got, ref.float(), TOL, "hswish forward")
        assert bool((got[x == -3.0] == 0).all()) and torch.equal(got[x == 3.0], x[x == 3.0]) and int((x == 3.0).sum()) > 0


def test_hswish_bn_bwd(backend):
    """bn_bwd's reduce and apply sweeps with hard-swish: the masked gradient against fp64 autograd through x * relu6(x + 3) / 6 (0 at -3 and
    below, dy at 3 and above), and dx / dgamma / dbeta with statistics that give scale 1 and shift 0 (tests/test_dwconv_kernels.py's scheme)."""
    x, dy, c = _hswish_inputs(backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    dg, db = torch.zeros(c, device=backend), torch.zeros(c, device=backend)
    dx, g = K.bn_bwd(to_nhwc(dy, backend), to_nhwc(x, backend), one, zero, one, zero, one, dg, db, act="hswish", want_g=True)
    xa = x.double().requires_grad_(True)
    (ga,) = torch.autograd.grad(hswish(xa), xa, dy.double())
    got = to_nchw_cpu(g)
    assert_close(got, ga.float(), TOL, "masked gradient")
    assert bool((got[x == -3.0] == 0).all()) and torch.equal(got[x == 3.0], dy[x == 3.0])
    M = x.numel() // c
    sg, sgx = ga.sum((0, 2, 3)), (ga * x.double()).sum((0, 2, 3))
    ref = ga - (sg / M).view(1, -1, 1, 1) - x.double() * (sgx / M).view(1, -1, 1, 1)
    assert_close(to_nchw_cpu(dx), ref.float(), TOL, "bn_bwd dx with hswish")
    assert_close(dg.cpu(), sgx.float(), 1e-4, "dgamma")
    assert_close(db.cpu(), sg.float(), 1e-4, "dbeta")


@pytest.mark.parametrize("stride", [1, 2])
def test_hswish_depthwise3x3_epilogue(backend, stride):
    n, h, w, c = (2, 9, 7, 32) if backend.type == "cuda" else (1, 4, 3, 16)
    g = torch.Generator().manual_seed(29)
    x, wt, bias = torch.randn(n, c, h, w, generator=g) * 2.0, torch.randn(c, 1, 3, 3, generator=g), torch.randn(c, generator=g)
    pre = F.conv2d(x.double(), wt.double(), bias.double(), stride, 1, groups=c)
    assert bool((pre < -3).any()) and bool((pre > 3).any()) and bool(((pre > -3) & (pre < 3)).any())
    y = K.dwconv3x3_fwd(to_nhwc(x, backend), K.to_dw(wt.to(backend)), bias=bias.to(backend), act="hswish", stride=stride)
    assert_close(to_nchw_cpu(y), hswish(pre).float(), TOL, "hswish(dwconv3x3 + bias)")


def test_hswish_is_rejected_where_it_is_not_implemented(backend):
    g = torch.Generator().manual_seed(1)
    x = to_nhwc(torch.randn(1, 16, 4, 4, generator=g), backend)
    ones = torch.ones(16, device=backend)
    with pytest.raises(_lib.SgxError, match="activation"):
        K.conv2d_fwd(x, K.to_ohwi(torch.randn(16, 16, 1, 1, generator=g).to(backend)), act="hswish")
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act(x, ones, ones, act="hswish")
    with pytest.raises(_lib.SgxError, match="activation"):
        K.tri_affine_act_bwd_reduce(x, x, ones, ones, ones, act="hswish")


# --------------------------------------------------------------------------------------------- BatchNorm -> gate -> activation
GATES = {"hardsigmoid": lambda p: F.relu6(p + 3.0) / 6.0, "none": lambda p: p}
GACTS = {"relu": F.relu, "hswish": hswish}


def _gate_case(shape, affine):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31 + h + c)
    x = torch.randn(n, c, h, w, generator=g) * 2.0
    pre = torch.randn(n, c, generator=g) * 2.5  # (gates on both sides of -3 and 3)
    scale = torch.rand(c, generator=g) + 0.5 if affine else None
    shift = torch.randn(c, generator=g) if affine else None
    dy, dmean, mean = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, generator=g), torch.randn(c, generator=g)
    return x, pre, scale, shift, dy, dmean, mean


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("act", ["relu", "hswish"])
@pytest.mark.parametrize("gate", ["hardsigmoid", "none"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 24), (2, 1, 1, 16)])
def test_gate_sweeps(backend, shape, gate, act, affine):
    """y = act(f(pre) * z), z = scale * x + shift, against an fp64 autograd composition; d pre and dz (= autograd's dz + dmean / HW); the
    reduce rows equal, bit for bit, what bn_bwd_reduce(dz, x, act = none) writes for the stored dz."""
    n, h, w, c = shape
    x, pre, scale, shift, dy, dmean, mean = _gate_case(shape, affine)
    xd, pd = x.double(), pre.double().requires_grad_(True)
    z = xd * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) if affine else xd.clone()
    z.requires_grad_(True)
    y = GACTS[act](GATES[gate](pd).view(n, c, 1, 1) * z)
    gz, gp = torch.autograd.grad(y, (z, pd), dy.double())
    dev = lambda t: None if t is None else t.to(backend)  # noqa: E731
    xk, dyk = to_nhwc(x, backend), to_nhwc(dy, backend)
    got = K.bn_gate_act_fwd(xk, dev(scale), dev(shift), dev(pre), gate, act=act)
    assert_close(to_nchw_cpu(got), y.detach().float(), TOL, "act(gate * z)")
    dpre = K.bn_gate_act_bwd_gate(dyk, xk, dev(scale), dev(shift), dev(pre), gate, act=act)
    assert_close(dpre.cpu(), gp.float(), 1e-4, "d pre")
    dz, parts = K.bn_gate_act_bwd_data(dyk, xk, dev(scale), dev(shift), dev(pre), gate, act=act, dmean=dev(dmean), save_mean=dev(mean), want_parts=True)
    assert_close(to_nchw_cpu(dz), (gz + dmean.double().view(n, c, 1, 1) / (h * w)).float(), TOL, "dz")
    plain = K.bn_gate_act_bwd_data(dyk, xk, dev(scale), dev(shift), dev(pre), gate, act=act)
    assert_close(to_nchw_cpu(plain), gz.float(), TOL, "dz without dmean and without rows")
    M = n * h * w
    rows = torch.empty(2, K.stats_blocks(M), c, device=backend)
    one, zero = torch.ones(c, device=backend), torch.zeros(c, device=backend)
    K.check(K.lib().sgx_bn_bwd_reduce(K.ptr(dz), c, K.ptr(xk), c, K.ptr(one), K.ptr(zero), K.ptr(dev(mean)), M, c, 0, K.ptr(rows), K.stream()), "sgx_bn_bwd_reduce")
    assert torch.equal(parts.cpu(), rows.cpu()), "reduce rows differ from bn_bwd_reduce's"


def test_gate_sweeps_reject_bad_arguments(backend):
    x = to_nhwc(torch.randn(1, 16, 2, 2, generator=torch.Generator().manual_seed(1)), backend)
    pre, ones = torch.zeros(1, 16, device=backend), torch.ones(16, device=backend)
    with pytest.raises(_lib.SgxError, match="scale and shift"):
        K.bn_gate_act_fwd(x, ones, None, pre, "hardsigmoid")
    with pytest.raises(_lib.SgxError, match="save_mean"):
        K.bn_gate_act_bwd_data(x, x, None, None, pre, "hardsigmoid", want_parts=True)
    L = K.lib()
    assert L.sgx_bn_gate_act_fwd(K.ptr(x), 16, None, None, K.ptr(pre), 7, K.ptr(x), 16, 1, 4, 16, 0, K.stream()) == -1
    assert L.sgx_bn_gate_act_fwd(K.ptr(x), 16, None, None, K.ptr(pre), 0, K.ptr(x), 16, 1, 4, 16, 5, K.stream()) == -1
    ws = torch.zeros(4, device=backend)
    assert L.sgx_bn_gate_act_bwd_gate(K.ptr(x), 16, K.ptr(x), 16, None, None, K.ptr(pre), 0, 0, K.ptr(pre), 1, 4, 16, K.ptr(ws), 16, K.stream()) == -4


# --------------------------------------------------------------------------------------------- dropout
def _philox(ctr, key):
    """Philox-4x32-10 (Salmon et al., SC'11) in plain Python: the four output words of one counter block."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_known_answers():
    """(Random123's kat_vectors for philox4x32 at ten rounds)"""
    assert _philox([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_dropout_mask_is_philox_of_seed_offset_and_element_index(backend):
    M, C, p, seed, offset = 5, 12, 0.3, (0x12345678 << 32) | 0x9ABCDEF0, (7 << 32) | 3
    x = torch.ones(M, C, device=backend)
    y = K.dropout(x, p, seed, offset).cpu()
    thresh = int(p * 2 ** 32)
    for r in range(M):
        for c4 in range(C // 4):
            words = _philox([(r * (C // 4) + c4) & 0xFFFFFFFF, 0, offset & 0xFFFFFFFF, offset >> 32], [seed & 0xFFFFFFFF, seed >> 32])
            for j in range(4):
                assert bool(y[r, c4 * 4 + j] != 0) == (words[j] >= thresh), (r, c4, j)


def test_dropout(backend):
    g = torch.Generator().manual_seed(37)
    N, C, p = 64, 1280, 0.2
    x = torch.randn(N, C, generator=g)
    x[x == 0] = 1.0
    xk = x.to(backend)
    assert torch.equal(K.dropout(xk, 0.0, 5).cpu(), x), "p = 0 is the identity, bit for bit"
    y = K.dropout(xk, p, 5).cpu()
    kept = y != 0
    assert torch.equal(y[kept], (x / torch.tensor(1.0 - p, dtype=torch.float32))[kept]), "kept values are x / (1 - p) exactly"
    sigma = math.sqrt(p * (1 - p) / (N * C))
    assert abs(float(kept.float().mean()) - (1 - p)) < 5 * sigma
    # the backward regenerates the mask; the mask does not depend on the launch geometry (a [64, 1280] matrix, the same elements as 4 x 16
    # pixel rows of an NHWC map, and rows with a stride)
    dy = torch.randn(N, C, generator=g)
    dy[dy == 0] = 1.0
    assert torch.equal(K.dropout(dy.to(backend), p, 5).cpu() != 0, kept), "backward mask"
    as_map = K.dropout(xk.view(4, 4, 4, C), p, 5).cpu().view(N, C)
    assert torch.equal(as_map, y), "NHWC view of the same elements"
    wide = torch.zeros(N, C + 8, device=backend)
    wide[:, 4: 4 + C] = xk
    assert torch.equal(K.dropout(wide[:, 4: 4 + C], p, 5).cpu(), y), "strided rows"
    narrow = K.dropout(xk.view(N * 20, 64), p, 5).cpu()  # 16 channel groups per row: another workgroup shape, the same group indices
    assert torch.equal(narrow.view(N, C), y), "another launch geometry"
    assert not torch.equal(K.dropout(xk, p, 5, offset=1).cpu() != 0, kept), "another offset, another mask"
    assert not torch.equal(K.dropout(xk, p, 6).cpu() != 0, kept), "another seed, another mask"
    with pytest.raises(_lib.SgxError, match="outside"):
        K.dropout(xk, 1.0, 5)
