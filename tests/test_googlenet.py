"""GoogLeNet: the Inception block (one output buffer, four slice-writing branches, the fused pool projection) and googlenet_v1 with its
ceil-mode pools, against the reference.

  reference (its own classification_models/googlenet.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/googlenet_*.pt elsewhere (tests/make_googlenet_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars.  The block: tests/test_blocks.py's - forward output, running statistics, eval output and folded-vs-unfolded eval at 2e-5, input and
parameter gradients at 1e-4.  The model (num_classes=10, dropout 0, 2 x 3 x S x S, deterministic_fill(seed=4)): training logits and
per-parameter gradient norms against the reference's fp64 run, no further from it than TWICE the reference's own fp32 run is - that distance
is computed when the fixture is written and stored in it (`bars`).  S = 64: the ceil-mode pools see 32 -> 16, 16 -> 8, 8 -> 4, 4 -> 2; S = 72:
36 -> 18 (floor mode: 17), 18 -> 9 (8), 9 -> 4, 4 -> 2 - the writer asserts the reference's extents.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc
from test_mobilenet import _check_grads, _record_step, _wrap

BLOCK_ARGS, BLOCK_SHAPE = (16, 8, 8, 16, 4, 8, 8), (2, 16, 5, 7)
SIZES = [64, 72]
EXTENTS = {64: [(32, 16), (16, 8), (8, 4), (4, 2)], 72: [(36, 18), (18, 9), (9, 4), (4, 2)]}  # (in, out) of maxpool1 .. maxpool4


def _block_input():
    return torch.randn(*BLOCK_SHAPE, generator=torch.Generator().manual_seed(1)) + 0.5


def _model_inputs(size):
    g = torch.Generator().manual_seed(5)
    return torch.randn(2, 3, size, size, generator=g), torch.randint(0, 10, (2,), generator=g)


def _grad_norm_errors(norms, t64):
    big = t64 > 1e-3 * t64.max()
    e = ((norms - t64).abs() / t64.clamp_min(1e-30))[big]
    return float(e.max()), float(e.mean())


# --------------------------------------------------------------------------------------------- reference side (recorded tensors)
def _block_reference():
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.googlenet as r

        torch.manual_seed(7)
        blk = torch.nn.Sequential(r.Inception(*BLOCK_ARGS))  # (keys 0.*: the product block is wrapped in a one-block network)
        G.deterministic_fill(blk, seed=11)
        return _record_step(blk, _block_input(), 5)

    return G.reference_outputs("googlenet_block_reference", compute)


def _model_reference(size):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.googlenet as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = r.GoogleNetV1(arch_params=HpmStruct(num_classes=10, dropout=0.0))
        G.deterministic_fill(ref, seed=4)
        layout = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        x, y = _model_inputs(size)
        ref64 = copy.deepcopy(ref).double()
        seen = []
        hooks = [getattr(ref, f"maxpool{i}").register_forward_hook(lambda m, a, o: seen.append((a[0].shape[2], o.shape[2]))) for i in (1, 2, 3, 4)]
        ref.train()
        ref64.train()
        logits = ref(x)
        assert seen == EXTENTS[size], seen
        for h in hooks:
            h.remove()
        F.cross_entropy(logits, y).backward()
        logits64 = ref64(x.double())
        F.cross_entropy(logits64, y).backward()
        names = [k for k, _ in ref.named_parameters()]
        p32, p64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
        n32 = torch.tensor([float(p32[k].grad.double().norm()) for k in names], dtype=torch.float64)
        n64 = torch.tensor([float(p64[k].grad.norm()) for k in names], dtype=torch.float64)
        worst, mean = _grad_norm_errors(n32, n64)
        return dict(state_layout=layout, logits_f64=logits64.detach(), grad_names=names, grad_norms_f64=n64,
                    bars=dict(logits=rel_err(logits.detach().double(), logits64.detach()), grad_worst=worst, grad_mean=mean))

    return G.reference_outputs(f"googlenet_v1_{size}_reference", compute)


# --------------------------------------------------------------------------------------------- the block
def test_inception_block_against_reference(backend):
    """Training forward into one buffer, input gradient (branch 1 writes, three accumulate), every parameter gradient, the running statistics
    of the six BatchNorms, eval forward, and the folded eval form (branch 4: bias and ReLU in the fused kernel's epilogue)."""
    from super_gradients_amd.training.models.classification_models.googlenet import Inception, PoolProjLayer

    fx = _block_reference()
    blk = Inception(*BLOCK_ARGS)
    net = _wrap([blk], backend)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in fx["state"].items()]
    assert isinstance(blk.branch4._modules["1"].conv, PoolProjLayer)
    net.load_state_dict(fx["state"], strict=True)
    net.train()
    net.zero_grad()
    x = to_nhwc(_block_input(), backend)
    y = blk.fwd(x)
    assert y.is_contiguous() and y.shape[3] == 40
    assert_close(to_nchw_cpu(y), fx["y"], 2e-5, "training forward")
    dy = to_nhwc(fx["dy"], backend)
    dy0 = dy.clone()
    dx = blk.bwd(dy)
    net.join_side()
    assert torch.equal(dy.cpu(), dy0.cpu()), "bwd changed the caller's dy"
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(net, fx, 1e-4)
    for k, b in net.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 2e-5, k)
    net.eval()
    with torch.no_grad():
        ye = to_nchw_cpu(blk.fwd(x))
        assert_close(ye, fx["y_eval"], 2e-5, "eval forward")
        net.prep_model_for_conversion()
        assert blk.branch4._modules["1"]._folded is not None
        assert_close(to_nchw_cpu(blk.fwd(x)), ye, 2e-5, "folded against unfolded eval forward")


# --------------------------------------------------------------------------------------------- the model
def test_state_dict_layout_helpers_and_refusals():
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.googlenet import GoogLeNet

    net = models.get("googlenet_v1", num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in _model_reference(64)["state_layout"]]
    assert net.fc.out_features == 10 and net.dropout.p == 0.3 and net.get_input_channels() == 3 and not net.supports_half_inference()
    assert models.get("googlenet_v1", arch_params=dict(num_classes=7, dropout=0.1)).dropout.p == 0.1
    assert net.gradient_buckets()[:4] == ["conv1.", "conv2.", "conv3.", "inception3a."] and net.gradient_buckets()[-1] == "fc."
    assert net.get_finetune_lr_dict(0.1) == {"fc": 0.1, "default": 0}
    w = net.inception4a.branch4._modules["1"].conv.weight
    assert float(w.detach().abs().max()) <= 0.02 and 0.007 < float(w.detach().std()) < 0.01  # trunc_normal_(std=0.01, a=-0.02, b=0.02): std 0.0088
    for kw in (dict(aux_logits=True), dict(aux_logits=False, backbone_mode=True)):
        with pytest.raises(NotImplementedError):
            GoogLeNet(**kw)
    with pytest.raises(NotImplementedError, match="new_head"):
        net.replace_head(new_head=torch.nn.Linear(1024, 2))


def _product_against_reference(size, device):
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    fx = _model_reference(size)
    net = models.get("googlenet_v1", arch_params=dict(dropout=0.0), num_classes=10)
    G.deterministic_fill(net, seed=4)
    net.materialize(device).train()
    x, y = _model_inputs(size)
    logits = net(x.to(device))
    CrossEntropyLoss()(logits, y.to(device)).backward()
    e = rel_err(logits.cpu().double(), fx["logits_f64"])
    params = dict(net.named_parameters())
    worst, mean = _grad_norm_errors(torch.tensor([float(params[n].grad.double().norm()) for n in fx["grad_names"]], dtype=torch.float64), fx["grad_norms_f64"])
    b = fx["bars"]
    print(f"googlenet_v1 at {size}: against the reference's fp64 run: logits {e:.2e} (reference fp32 {b['logits']:.2e}), gradient norms worst {worst:.2e} "
          f"({b['grad_worst']:.2e}) mean {mean:.2e} ({b['grad_mean']:.2e})")
    assert e <= 2 * b["logits"] and worst <= 2 * b["grad_worst"] and mean <= 2 * b["grad_mean"]


@pytest.mark.parametrize("size", SIZES)
def test_product_googlenet_emulation(size):
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference(size, torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_product_googlenet_golden(gpu_device, size):
    _product_against_reference(size, gpu_device)
