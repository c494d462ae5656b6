"""seg_ce (CrossEntropyLoss on an NCHW map) against fp64 F.cross_entropy, and seg_confusion against a torch.bincount restatement.

Shapes (N, C, H, W): (2, 19, 4, 5) P % 4 == 0, under one workgroup, two images; (2, 19, 3, 7) P % 4 != 0, unaligned planes, the scalar path;
(1, 3, 33, 37) several workgroups with a ragged last one; (1, 32, 4, 6) / (1, 33, 4, 6) either side of the register / streaming cut
(SEG_CE_REG_CAP = 32); (2, 40, 3, 7) streaming on the scalar path.
Bar of the loss and of the logits' gradient: TWICE the distance of ATen's own fp32 F.cross_entropy (CPU) from the fp64 result on the same
inputs - two correct fp32 implementations differ by about each one's own error (tests/test_regseg.py's margin) - with a floor of 4 fp32
epsilons of the fp64 value (of the largest gradient element), for the cases where ATen happens to round exactly: each implementation makes at
least an exp, a log or divide and a multiply by the weight or 1 / denominator per element, every one correct to about one epsilon.
Measured distances (loss relative, gradient relative to its largest element): DESIGN.md 26.5."""
import pytest
import torch
import torch.nn.functional as F

EPS = torch.finfo(torch.float32).eps
S_VEC, S_SCALAR, S_MULTI, S_CAP, S_OVER, S_STREAM = (2, 19, 4, 5), (2, 19, 3, 7), (1, 3, 33, 37), (1, 32, 4, 6), (1, 33, 4, 6), (2, 40, 3, 7)
# option sets: ignore_index (None = the default -100, no ignored pixel), per-class weights, reduction, what to overwrite with ignore_index
IGN19, IGN0, PLAIN, W_MEAN, W_SUM = (19, False, "mean", "third"), (0, False, "mean", None), (None, False, "mean", None), (None, True, "mean", None), (
    19, True, "sum", "third")
CE_CASES = [(S_VEC, IGN19), (S_VEC, W_MEAN), (S_SCALAR, IGN19), (S_SCALAR, W_SUM), (S_MULTI, IGN0), (S_MULTI, PLAIN), (S_CAP, PLAIN), (S_CAP, W_SUM),
            (S_OVER, IGN0), (S_OVER, W_MEAN), (S_STREAM, IGN19), (S_STREAM, W_SUM),
            (S_VEC, (19, False, "mean", "image")), (S_VEC, (19, True, "mean", "all"))]


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    return 3.0 * torch.randn(shape, generator=g), torch.randint(0, c, (n, h, w), generator=g), 0.5 + torch.rand(c, generator=g)


@pytest.mark.parametrize("shape,opts", CE_CASES)
def test_seg_ce_against_fp64(backend, shape, opts):
    from super_gradients_amd.training.losses import CrossEntropyLoss

    ignore, weighted, reduction, hide = opts
    x, y, w = _inputs(shape)
    if hide == "third":
        y.view(-1)[::3] = ignore
    elif hide == "image":
        y[0] = ignore
    elif hide == "all":
        y[:] = ignore
    kw = dict(reduction=reduction, **({} if ignore is None else {"ignore_index": ignore}))

    def aten(dtype):
        xr = x.to(dtype).clone().requires_grad_()
        loss = F.cross_entropy(xr, y, weight=w.to(dtype) if weighted else None, **kw)
        loss.backward()
        return loss.detach().double(), xr.grad.double()

    (l64, g64), (l32, g32) = aten(torch.float64), aten(torch.float32)
    runs = []
    for _ in range(2):
        xd = x.clone().to(backend).requires_grad_()
        loss = CrossEntropyLoss(weight=w if weighted else None, **kw)(xd, y.to(backend))
        loss.backward()
        runs.append((loss.detach().cpu(), xd.grad.cpu()))
    (loss, grad), (loss2, grad2) = runs
    # bit-repeatable (fixed-order reductions, no float atomics); compared as bits, so that the all-ignored nan compares too
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    if hide == "all":
        assert loss.isnan() and l64.isnan()
        return
    gmax = g64.abs().max()
    e_loss, e_grad = (loss.double() - l64).abs(), (grad.double() - g64).abs().max()
    bar_loss, bar_grad = max(2 * (l32 - l64).abs(), 4 * EPS * l64.abs()), max(2 * (g32 - g64).abs().max(), 4 * EPS * gmax)
    print(f"{shape} {opts}: loss err {float(e_loss / l64.abs()):.2e} (ATen fp32 {float((l32 - l64).abs() / l64.abs()):.2e}), "
          f"grad err {float(e_grad / gmax):.2e} (ATen fp32 {float((g32 - g64).abs().max() / gmax):.2e})")
    assert loss.isfinite() and e_loss <= bar_loss and e_grad <= bar_grad
    if hide == "image":
        assert not grad[0].any() and grad[1].any()
    if ignore is not None:
        assert not grad.permute(0, 2, 3, 1)[y == ignore].any()  # zero in every class plane of an ignored pixel


def test_seg_ce_rejects_label_smoothing(backend):
    from super_gradients_amd.training.losses import CrossEntropyLoss

    x, y, _ = _inputs(S_VEC)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(smooth_eps=0.1)(x.to(backend), y.to(backend))


@pytest.mark.parametrize("extra_bins,ignore", [(0, ()), (1, (3,)), (0, (3, 255)), (120, (3,))])  # (+120 bins: an LDS matrix beyond 64 KB)
@pytest.mark.parametrize("shape", [S_VEC, S_SCALAR, S_MULTI, S_STREAM])
def test_seg_confusion_exact(backend, shape, extra_bins, ignore):
    from super_gradients_amd import kernels as K

    x, y, _ = _inputs(shape, seed=1)
    nb = shape[1] + extra_bins
    y = torch.randint(0, nb + 1, y.shape, generator=torch.Generator().manual_seed(2))  # nb itself: the out-of-range row
    y.view(-1)[::5] = 3
    y.view(-1)[1::7] = 255
    pred, lab = x.double().argmax(1).reshape(-1), y.reshape(-1)
    keep = ~torch.isin(lab, torch.tensor(ignore, dtype=torch.long))
    row = torch.where((lab >= 0) & (lab < nb), lab, torch.full_like(lab, nb))
    ref = torch.bincount(row[keep] * nb + pred[keep], minlength=(nb + 1) * nb).reshape(nb + 1, nb)
    counts = K.seg_confusion(x.to(backend), y.to(backend), nb, ignore)
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), ref)
    again = K.seg_confusion(x.to(backend), y.to(backend), nb, ignore, counts=counts)  # accumulates
    assert again is counts and torch.equal(counts.cpu(), 2 * ref)


def test_seg_confusion_rejects_bins_above_the_lds_cap(backend):
    from super_gradients_amd import _lib
    from super_gradients_amd import kernels as K

    x, y, _ = _inputs(S_VEC)
    with pytest.raises(_lib.SgxError):
        K.seg_confusion(x.to(backend), y.to(backend), 193)
