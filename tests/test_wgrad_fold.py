"""The fold tree of the grouped weight gradient (wgrad_kernel in conv.hip, wpatch_kernel in wgrad_patch.hip): a workgroup LOOKS at its
pair's ticket before it publishes its node and writes nothing where the sibling is already there, and a ticket counts only if it holds
the launch epoch of the call - no call clears its tickets.  Neither touches the arithmetic: every node stays left + right of the same two
children, so the results must be bit-identical to the form that always publishes and clears per call (sgx_debug_set_wgrad_fold(1)),
whatever order the workgroups arrive in, and whatever an earlier call left in the ticket buffer."""
import ctypes
from contextlib import contextmanager

import torch
import torch.nn.functional as F

from util import assert_close, to_nhwc

from super_gradients_amd import kernels as K

TOL = 2e-5  # the convolution tolerance of test_kernels.py (max error relative to the largest reference entry)

# (N, H, W, C, K, R, stride, pad)
GPU_CASES = [(2, 80, 80, 64, 64, 3, 1, 1),    # patch kernel, stride 1
             (4, 40, 40, 32, 48, 3, 2, 1),    # patch kernel, stride 2
             (2, 80, 80, 96, 96, 1, 1, 0),    # slab loop, 96-wide tile
             (1, 20, 20, 128, 32, 1, 1, 0),   # two splits
             (2, 160, 160, 4, 48, 3, 2, 1)]
EMU_CASES = [(1, 42, 42, 4, 8, 1, 1, 0),      # 1764 pixels, 7 splits of 256: a three-level tree with sibling-less nodes
             (1, 9, 7, 8, 36, 3, 1, 1),
             (2, 12, 12, 8, 8, 3, 2, 1),
             (2, 34, 36, 4, 8, 3, 2, 1)]
# Sibling pairs of the emulation cases under the small items of `_small_items`: a tree over n splits has n - 1 pairs per dW tile.
#   case 0: slab loop, one 32 x 32 dW tile, 1764 pixels in items of (at least) 256 -> 7 splits -> 6 pairs
#   case 1: 63 output pixels, case 2: 72 - fewer than one item of 256 pixels: ONE split, no pair (direct accumulate)
#   case 3: patch kernel (3x3, pad 1, stride 2): 17 x 18 outputs in tiles of 4 x 8 -> 5 x 3 tiles x 2 images = 30 tiles of 32 pixels,
#           items of at least 8 tiles (256 pixels) -> 4 ranges (of 8, 8, 8, 6 tiles) -> 3 pairs; one dW tile (8 filters x 4 channels)
EMU_PAIRS = 6 + 0 + 0 + 3

_HOST = {}


def _host_cases(gpu):
    """CPU inputs and ATen's weight gradients of the case list, computed once per process and never modified."""
    if gpu not in _HOST:
        out = []
        for i, shape in enumerate(GPU_CASES if gpu else EMU_CASES):
            n, h, w, c, k, r, s, p = shape
            g = torch.Generator().manual_seed(300 + i)
            x = torch.randn(n, c, h, w, generator=g)
            wt = (torch.randn(k, c, r, r, generator=g) / (c * r * r) ** 0.5).requires_grad_(True)
            y = F.conv2d(x, wt, None, stride=s, padding=p)
            dy = torch.randn(y.shape, generator=g)
            y.backward(dy)
            out.append((shape, x, dy, wt.grad.detach()))
        _HOST[gpu] = out
    return _HOST[gpu]


def _entries(backend, which=None):
    """[(x, dy, dw, stride, pad)] on the backend - the operands are channel slices of wider buffers - and the references."""
    host = _host_cases(backend.type == "cuda")
    if which is not None:
        host = [host[i] for i in which]
    ents, refs, shapes = [], [], []
    for shape, x, dy, ref in host:
        n, h, w, c, k, r, s, p = shape
        ents.append((to_nhwc(x, backend, ld_pix=c + 8, c_off=4), to_nhwc(dy, backend, ld_pix=k + 4, c_off=0), K.ohwi_empty(k, c, r, r, backend), s, p))
        refs.append(ref)
        shapes.append(shape)
    return ents, refs, shapes


@contextmanager
def _small_items():
    """Small work items, so that every tree has several levels; every 3x3 pad-1 job takes the patch kernel (as test_wgrad_patch_kernel)."""
    from super_gradients_amd._lib import lib

    try:
        lib().sgx_debug_set_wgrad_group(6, 1, 1)
        lib().sgx_debug_set_wgrad_patch(1, 0, 1)
        lib().sgx_debug_set_wgrad_fold(0)
        yield lib()
    finally:
        lib().sgx_debug_set_wgrad_group(0, 0, 1)
        lib().sgx_debug_set_wgrad_patch(0, 0, 0)
        lib().sgx_debug_set_wgrad_fold(0)


def _run(ents, fill=0.25):
    for e in ents:
        e[2].fill_(fill)
    K.conv2d_bwd_weight_group(ents)
    return [e[2].cpu().clone() for e in ents]


def _counts(library, reset=True):
    pub, skip = ctypes.c_int64(), ctypes.c_int64()
    assert library.sgx_debug_wgrad_fold_counts(ctypes.byref(pub), ctypes.byref(skip), int(reset)) == 0
    return pub.value, skip.value


def test_fold_modes_agree_bit_for_bit(backend, monkeypatch):
    """Look + epoch (mode 0) against always-publish + clear-per-call (mode 1): torch.equal on every dw; both agree with ATen."""
    ents, refs, shapes = _entries(backend)
    if backend.type != "cuda":
        monkeypatch.setenv("SGX_EMU_SHUFFLE", "7")
    with _small_items() as library:
        got = {}
        for mode in (1, 0, 1, 0):  # (interleaved: each form also runs on the tickets the other one left)
            library.sgx_debug_set_wgrad_fold(mode)
            out = _run(ents)
            if mode in got:
                for shape, a, b in zip(shapes, got[mode], out):
                    assert torch.equal(a, b), f"fold mode {mode}, second run differs {shape}"
            got[mode] = out
        for shape, a, b, ref in zip(shapes, got[0], got[1], refs):
            assert torch.equal(a, b), f"fold modes 0 and 1 differ {shape}"
            assert_close(a, ref + 0.25, TOL, f"fold mode 0 {shape}")
            assert_close(b, ref + 0.25, TOL, f"fold mode 1 {shape}")


def test_arrival_order_does_not_matter(backend, monkeypatch):
    """Another arrival order (the emulation dispatches the workgroups shuffled by a seed; on the chip: the plain block order instead of the
    XCD-aware one, and a repeated launch) gives the same bits - which of a pair looks and which publishes changes, the sum does not."""
    gpu = backend.type == "cuda"
    ents, refs, shapes = _entries(backend)
    with _small_items() as library:
        outs = []
        for seed, xcd in (("7", 1), ("1234", 0), ("99", 1)):
            if not gpu:
                monkeypatch.setenv("SGX_EMU_SHUFFLE", seed)
            library.sgx_debug_set_wgrad_group(6, 1, xcd)
            outs.append(_run(ents))
        for shape, a, b, c, ref in zip(shapes, outs[0], outs[1], outs[2], refs):
            assert torch.equal(a, b) and torch.equal(a, c), f"the fold must not depend on the arrival order {shape}"
            assert_close(a, ref + 0.25, TOL, f"grouped wgrad {shape}")


def test_no_clear_needed(backend, monkeypatch):
    """Calls in a row on ONE ticket buffer with nothing cleared in between: three calls (dw = 0.25 + i ref after call i), a fourth on a
    buffer poisoned with 0x7fffffff, a fifth on one poisoned with -1, then another job list (another plan: other ticket offsets) on the
    same buffer."""
    gpu = backend.type == "cuda"
    ents, refs, shapes = _entries(backend)
    if not gpu:
        monkeypatch.setenv("SGX_EMU_SHUFFLE", "5")
    with _small_items():
        for e in ents:
            e[2].fill_(0.25)
        K.conv2d_bwd_weight_group(ents)
        key = (backend, K.stream() or 0)
        tk = K._TICKETS[key]
        for i in range(1, 6):
            if i > 1:
                K.conv2d_bwd_weight_group(ents)
            assert K._TICKETS[key] is tk, "the calls must share one ticket buffer"
            for shape, e, ref in zip(shapes, ents, refs):
                assert_close(e[2].cpu(), 0.25 + i * ref, TOL, f"call {i} on uncleared tickets {shape}")
            if i == 3:
                tk.fill_(0x7fffffff)
            if i == 4:
                tk.fill_(-1)
        # another plan on the same buffer: the jobs in reverse order without the first one - other tiles, splits and ticket offsets
        which = list(range(len(shapes)))[:0:-1]
        ents2, refs2, shapes2 = _entries(backend, which)
        out = _run(ents2)
        assert K._TICKETS[key] is tk
        for shape, a, ref in zip(shapes2, out, refs2):
            assert_close(a, 0.25 + ref, TOL, f"another job list on the same tickets {shape}")
        # ... and the first list again, on what that left
        out = _run(ents)
        for shape, a, ref in zip(shapes, out, refs):
            assert_close(a, 0.25 + ref, TOL, f"first job list after another plan {shape}")


def test_publication_counts(backend, monkeypatch):
    """The emulation runs the workgroups one after another, so the second arriver of every pair finds its sibling there: with the look,
    published nodes == sibling pairs == skipped nodes, exactly; under mode 1 every node of a pair is published (twice the pairs) and none
    is skipped.  The product kernels carry no counter (the getter says -1)."""
    ents, refs, shapes = _entries(backend)
    with _small_items() as library:
        if backend.type == "cuda":
            _run(ents)
            assert _counts(library) == (-1, -1)
            return
        for seed in ("3", "77"):
            monkeypatch.setenv("SGX_EMU_SHUFFLE", seed)
            _counts(library)
            library.sgx_debug_set_wgrad_fold(0)
            _run(ents)
            assert _counts(library) == (EMU_PAIRS, EMU_PAIRS), f"look: published, skipped (shuffle seed {seed})"
            library.sgx_debug_set_wgrad_fold(1)
            _run(ents)
            assert _counts(library) == (2 * EMU_PAIRS, 0), f"always publish: published, skipped (shuffle seed {seed})"


def test_single_split_and_mixed_group(backend, monkeypatch):
    """Default item sizes: every job of these lists is a single split or nearly so (direct accumulate, no ticket touched), under both fold
    modes; and a group that mixes patch-kernel and slab-loop jobs, one job at a time against the group (each job's tree is its own)."""
    gpu = backend.type == "cuda"
    ents, refs, shapes = _entries(backend)
    from super_gradients_amd._lib import lib

    if not gpu:
        monkeypatch.setenv("SGX_EMU_SHUFFLE", "21")
    try:
        for mode in (0, 1):
            lib().sgx_debug_set_wgrad_fold(mode)
            out = _run(ents, fill=0.0)
            for shape, a, ref in zip(shapes, out, refs):
                assert_close(a, ref, TOL, f"default items, fold mode {mode} {shape}")
    finally:
        lib().sgx_debug_set_wgrad_fold(0)
    with _small_items():
        grouped = _run(ents)
        for j, (shape, ref) in enumerate(zip(shapes, refs)):
            alone = _run([ents[j]])[0]
            assert_close(alone, ref + 0.25, TOL, f"one job alone {shape}")
            if not gpu:  # (on the emulation the small items do not depend on the group: the same splits, the same tree, the same bits)
                assert torch.equal(alone, grouped[j]), f"a job alone and inside the mixed group {shape}"
