"""OhemCELoss / DDRNetLoss (kernels.seg_ohem_ce, csrc/seg_ohem.h) against a plain-torch restatement of the reference's OhemLoss.forward, run in
fp64 for the value and in fp32 for the bar.

Shapes (N, C, H, W): (2, 19, 4, 5) 16-byte path under one workgroup; (2, 19, 3, 7) scalar path; (1, 3, 33, 37) several workgroups with a ragged
last one and chunks without a selected pixel; (1, 33, 4, 6) the streaming form.  Modes: `bar` (threshold 0.7: more than num_mining losses above
it), `topk` (threshold 1e-4, thresh = 9.2: the rank decides), each with every third label ignored and the ignored pixels excluded from or left
in the set, and `deep` (logits * 1e-3: every loss is ln C +- 0.01, so the second and third radix levels decide the rank; on the 1221-pixel
shape neighbours in the sorted losses lie about 6e-6 apart except at the very top, so the input condition can only hold for a small rank:
num_mining = 3 there, 30 % of the pixels on the small shapes).
Bar (tests/test_segloss_kernels.py's): loss and gradient within TWICE the fp32 restatement's own distance from fp64, floor 4 fp32 epsilons.
Input condition, asserted on the restatements alone: fp64 and fp32 select the same pixels, and the fp64 losses keep a relative gap of 1e-4 from
thresh and between sorted[num_mining - 1] and sorted[num_mining]; SEEDS holds a seed per case for which it holds."""
import pytest
import torch
import torch.nn.functional as F

EPS = torch.finfo(torch.float32).eps
IGN = 255
SHAPES = [(2, 19, 4, 5), (2, 19, 3, 7), (1, 3, 33, 37), (1, 33, 4, 6)]
# mode: (threshold, mining_percent, logit scale, ignore every third label, exclude ignored pixels from the set)
MODES = {"bar": (0.7, 0.1, 3.0, False, True), "bar_excl": (0.7, 0.1, 3.0, True, True), "bar_incl": (0.7, 0.1, 3.0, True, False),
         "topk": (1e-4, 0.5, 3.0, False, True), "topk_excl": (1e-4, 0.5, 3.0, True, True), "topk_incl": (1e-4, 0.5, 3.0, True, False),
         "deep": (1e-4, None, 3e-3, False, True)}
SEEDS = {((2, 19, 4, 5), "deep"): 1, ((2, 19, 3, 7), "deep"): 2, ((1, 33, 4, 6), "deep"): 4}  # (shape, mode) -> seed meeting the input condition; 0 where absent


def _case(shape, mode):
    threshold, percent, scale, hide, exclude = MODES[mode]
    npix = shape[0] * shape[2] * shape[3]
    return threshold, percent or (0.3 if npix < 100 else 3.5 / npix), scale, hide, exclude


def _inputs(shape, scale, hide, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x, y = scale * torch.randn(shape, generator=g), torch.randint(0, c, (n, h, w), generator=g)
    if hide:
        y.view(-1)[::3] = IGN
    return x, y


def _restated(x, y, threshold, percent, exclude, dtype):
    """OhemLoss.forward -> (loss, gradient, per-pixel losses of the set sorted descending, num_mining, selected-pixel mask)"""
    xr = x.to(dtype).clone().requires_grad_()
    pix = F.cross_entropy(xr, y, ignore_index=IGN, reduction="none").view(-1)
    keep = y.view(-1) != IGN if exclude else torch.ones_like(y.view(-1), dtype=torch.bool)
    loss = pix[keep]
    num_mining = min(int(percent * loss.numel()), loss.numel() - 1)
    thresh = (-torch.log(torch.tensor(threshold, dtype=torch.float))).to(dtype)
    srt, order = torch.sort(loss, descending=True)
    chosen = order[srt > thresh] if srt[num_mining] > thresh else order[:num_mining]
    out = loss[chosen].mean()
    out.backward()
    mask = torch.zeros(y.numel(), dtype=torch.bool)
    mask[keep.nonzero().view(-1)[chosen]] = True
    return out.detach().double(), xr.grad.double(), srt.detach().double(), num_mining, mask, float(thresh)


def _run(backend, x, y, **kw):
    from super_gradients_amd.training.losses import OhemCELoss

    xd = x.clone().to(backend).requires_grad_()
    loss = OhemCELoss(ignore_lb=IGN, **kw)(xd, y.to(backend))
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


def _within_bar(loss, grad, l64, g64, l32, g32):
    gmax = g64.abs().max()
    e_loss, e_grad = (loss.double() - l64).abs(), (grad.double() - g64).abs().max()
    print(f"loss err {float(e_loss / l64.abs()):.2e} (fp32 restatement {float((l32 - l64).abs() / l64.abs()):.2e}), "
          f"grad err {float(e_grad / gmax):.2e} (fp32 restatement {float((g32 - g64).abs().max() / gmax):.2e})")
    assert loss.isfinite() and e_loss <= max(2 * (l32 - l64).abs(), 4 * EPS * l64.abs())
    assert e_grad <= max(2 * (g32 - g64).abs().max(), 4 * EPS * gmax)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES)
def test_ohem_ce_against_fp64(backend, shape, mode):
    threshold, percent, scale, hide, exclude = _case(shape, mode)
    x, y = _inputs(shape, scale, hide, SEEDS.get((shape, mode), 0))
    l64, g64, s64, k, mask64, thresh = _restated(x, y, threshold, percent, exclude, torch.float64)
    l32, g32, _, _, mask32, _ = _restated(x, y, threshold, percent, exclude, torch.float32)
    # the input condition: one pixel set in both precisions, no loss within 1e-4 (relative) of either decision
    assert k > 0 and torch.equal(mask64, mask32)
    assert ((s64 - thresh).abs() >= 1e-4 * thresh).all() and s64[k - 1] - s64[k] >= 1e-4 * s64[k - 1]
    assert (s64[k] > thresh) == mode.startswith("bar")  # the case takes the branch it is named for
    kw = dict(threshold=threshold, mining_percent=percent, num_pixels_exclude_ignored=exclude)
    (loss, grad), (loss2, grad2) = _run(backend, x, y, **kw), _run(backend, x, y, **kw)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    _within_bar(loss, grad, l64, g64, l32, g32)
    assert not grad.permute(0, 2, 3, 1).reshape(-1, shape[1])[~mask64].any()  # zero in every plane of an unselected or ignored pixel


def test_ohem_ce_tie_across_the_rank_boundary(backend):
    """Four bit-equal pixels (one logit column, one label) hold the largest loss and num_mining = 2 cuts through them: the value is that
    loss, the weights sum to 1 and the four share them equally."""
    x, y = _inputs(SHAPES[0], 3.0, False, 0)
    pix = F.cross_entropy(x.double(), y, reduction="none")
    n, h, w = (int(v) for v in (pix == pix.max()).nonzero()[0])
    for hh, ww in ((0, 0), (1, 2), (2, 3), (3, 4)):
        x[n, :, hh, ww], y[n, hh, ww] = x[n, :, h, w], y[n, h, w]
    kw = dict(threshold=1e-9, mining_percent=2.5 / y.numel(), num_pixels_exclude_ignored=True)  # num_mining = 2; thresh = 20.7, above every loss
    l64, g64, s64, k, _, thresh = _restated(x, y, 1e-9, kw["mining_percent"], True, torch.float64)
    l32, g32 = _restated(x, y, 1e-9, kw["mining_percent"], True, torch.float32)[:2]
    assert k == 2 and s64[0] == s64[3] > s64[4] and s64[0] < thresh
    loss, grad = _run(backend, x, y, **kw)
    assert (loss.double() - l64).abs() <= max(2 * (l32 - l64).abs(), 4 * EPS * l64.abs())
    weight = -grad.gather(1, y.unsqueeze(1)).squeeze(1).double() / (1 - F.softmax(x.double(), 1).gather(1, y.unsqueeze(1)).squeeze(1))
    tied = F.cross_entropy(x, y, reduction="none") == F.cross_entropy(x, y, reduction="none").max()
    assert int(tied.sum()) >= 4 and abs(float(weight.sum()) - 1) <= 8 * EPS
    assert (weight[tied] == weight[tied][0]).all() and not grad.permute(0, 2, 3, 1)[~tied].any()


def test_ohem_ce_nothing_to_mine_is_nan_with_zero_gradient(backend):
    x, y = _inputs(SHAPES[0], 3.0, False, 0)
    loss, grad = _run(backend, x, y, threshold=1e-9, mining_percent=1e-3)  # int(0.001 * 40) = 0, no loss above thresh = 20.7
    assert loss.isnan() and loss.dim() == 0 and not grad.any()


def test_ohem_ce_all_ignored_is_zero(backend):
    x, y = _inputs(SHAPES[0], 3.0, False, 0)
    loss, grad = _run(backend, x, torch.full_like(y, IGN), threshold=0.7, num_pixels_exclude_ignored=True)
    assert loss == 0 and loss.dim() == 0 and not grad.any()


def test_ddrnet_loss_weights_two_predictions(backend):
    from super_gradients_amd.training.losses import DDRNetLoss, OhemCELoss

    (x1, y), (x2, _) = _inputs(SHAPES[0], 3.0, True, 0), _inputs(SHAPES[0], 3.0, True, 1)
    a, b = (OhemCELoss(0.7, 0.1, IGN, False)(x.to(backend), y.to(backend)).cpu() for x in (x1, x2))
    crit = DDRNetLoss()
    p1, p2 = x1.clone().to(backend).requires_grad_(), x2.clone().to(backend).requires_grad_()
    total, items = crit([p1, p2], y.to(backend))
    total.backward()
    assert len(crit.component_names) == 3 and not items.requires_grad
    assert torch.allclose(total.detach().cpu(), 1.0 * a + 0.4 * b, rtol=4 * EPS, atol=0)
    assert torch.equal(items.cpu(), torch.stack([a, b, total.detach().cpu()]))
    assert p1.grad.any() and p2.grad.any()
    single, _ = DDRNetLoss(weights=[1.0])(x1.to(backend), y.to(backend))  # a tensor stands for a list of one
    assert torch.equal(single.cpu(), a)


@pytest.mark.parametrize("name,params", [("DDRNetLoss", {}), ("OhemCELoss", {"threshold": 0.7})])
def test_trainer_resolves_ohem_losses_by_name(name, params):
    from super_gradients_amd.training import losses
    from super_gradients_amd.training.sg_trainer.sg_trainer import Trainer

    tp = type("TP", (), {"loss": name, "criterion_params": params})()
    assert type(Trainer._build_loss(None, tp)) is getattr(losses, name)
