"""MobileNetV3 classifiers: the inverted-residual block in both layouts (depthwise 3x3 / 5x5, squeeze-excitation before or after the
activation, ReLU / hard-swish), the mobilenet_v3 models, dropout in the classifier and Trainer steps.

  reference (its own classification_models/mobilenetv3.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/mobilenetv3_*.pt elsewhere (tests/make_mobilenetv3_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars as tests/test_mobilenet.py.  A block: tests/test_blocks.py's `_check` - forward output, running statistics and eval output at 2e-5, input
and parameter gradients at 1e-4 (relative, max-norm).  A whole model (classifier.2.p = 0 on both sides): logits and loss at 1e-4, parameter
gradients by tests/test_resnet.py's `_grad_check`.  On this input (4 x 3 x 64 x 64, seed 5) the reference's own fp32 run is, against its
fp64 run (tests/make_mobilenetv3_golden.py prints it): logits 2.5e-6 (mobilenet_v3_large) / 1.5e-6 (mobilenet_v3_small), per-parameter
gradient norms overall 3.0e-6 / 1.8e-7 - far inside a third of the 1e-4 bar.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc

MODELS = ["mobilenet_v3_large", "mobilenet_v3_small"]
CLS = {"mobilenet_v3_large": "mobilenetv3_large", "mobilenet_v3_small": "mobilenetv3_small"}
# (inp, hidden_dim, oup, kernel_size, stride, use_se, use_hs): 3x3 without SE, ReLU, residual; 5x5 stride 2 with SE (between BatchNorm and
# ReLU); 5x5 with SE, hard-swish and residual; the inp == hidden_dim layout (SE after the activation) at stride 2
BLOCKS = {"k3res": (16, 64, 16, 3, 1, 0, 0), "k5s2se": (24, 72, 40, 5, 2, 1, 0), "k5sehs": (40, 120, 40, 5, 1, 1, 1), "same_se_s2": (16, 16, 24, 3, 2, 1, 0)}


def _block_input(c):
    return torch.randn(2, c, 6, 6, generator=torch.Generator().manual_seed(1)) + 0.5


def _record_step(mod, x, seed):
    mod.train()
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    xa = x.clone().requires_grad_(True)
    y = mod(xa)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed))
    y.backward(dy)
    out = dict(state=state, y=y.detach(), dy=dy, x_grad=xa.grad.clone(), grads={k: p.grad.clone() for k, p in mod.named_parameters()},
               buffers={k: v.clone() for k, v in mod.named_buffers() if not k.endswith("num_batches_tracked")})
    mod.eval()
    with torch.no_grad():
        out["y_eval"] = mod(x)
    return out


def _block_reference():
    def compute():
        ref_shim.install()
        from super_gradients.training.models.classification_models.mobilenetv3 import InvertedResidual as RefBlock

        out = {}
        for i, (name, cfg) in enumerate(BLOCKS.items()):
            torch.manual_seed(7 + i)
            blk = RefBlock(*cfg)
            G.deterministic_fill(blk, seed=11 + i)
            out[name] = _record_step(blk, _block_input(cfg[0]), 5 + i)
        return out

    return G.reference_outputs("mobilenetv3_block_reference", compute)


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)


def _model_reference(name):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.mobilenetv3 as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
        G.deterministic_fill(ref, seed=4)
        ref.classifier[2].p = 0.0
        layout = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        x, y = _model_inputs()
        ref64 = copy.deepcopy(ref).double()
        ref.train()
        ref64.train()
        logits = ref(x)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        logits64 = ref64(x.double())
        F.cross_entropy(logits64, y).backward()
        names = [k for k, _ in ref.named_parameters()]
        p32, p64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
        checks = {k: float(v.double().sum()) for k, v in ref.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")}
        ref.eval()
        with torch.no_grad():
            eval_logits = ref(x)
        return dict(state_layout=layout, logits=logits.detach(), loss=loss.detach(), logits_f64=logits64.detach(), grad_names=names,
                    grad_norms=torch.tensor([float(p32[k].grad.double().norm()) for k in names], dtype=torch.float64),
                    grad_norms_f64=torch.tensor([float(p64[k].grad.norm()) for k in names], dtype=torch.float64),
                    bn_running_checksum=checks, eval_logits=eval_logits)

    return G.reference_outputs(f"mobilenetv3_{name}_reference", compute)


# --------------------------------------------------------------------------------------------- blocks
def _wrap(blocks, device):
    from super_gradients_amd.modules.engine import SgxNetwork

    class Net(SgxNetwork):
        def __init__(self):
            super().__init__()
            for i, b in enumerate(blocks):
                self.add_module(str(i), b)

    net = Net()
    net.materialize(device)
    return net


def _check_grads(net, fx, tol):
    gmax = max(float(g.abs().max()) for g in fx["grads"].values())
    for name, p in net.named_parameters():
        rg = fx["grads"][name]
        e = float((p.grad.cpu().double().reshape(rg.shape) - rg.double()).abs().max()) / max(float(rg.abs().max()), 1e-2 * gmax)
        assert e <= tol, f"grad {name}: {e:.3e}"


@pytest.mark.parametrize("cfg", list(BLOCKS))
def test_inverted_residual_against_reference(backend, cfg):
    """The product block against the reference's InvertedResidual: training forward, input gradient, every parameter gradient (the SE weights
    and the 5x5 filter included), running statistics after the step, eval forward, and the folded eval form against the unfolded one."""
    from super_gradients_amd.modules.layers import DepthwiseConvLayer
    from super_gradients_amd.modules.se_blocks import SELayer
    from super_gradients_amd.training.models.classification_models.mobilenetv3 import InvertedResidual

    inp, hidden, oup, k, stride, use_se, use_hs = BLOCKS[cfg]
    fx = _block_reference()[cfg]
    blk = InvertedResidual(*BLOCKS[cfg])
    assert list(blk.state_dict().keys()) == list(fx["state"].keys())
    assert [tuple(v.shape) for v in blk.state_dict().values()] == [tuple(v.shape) for v in fx["state"].values()]
    dws = [m for m in blk.modules() if isinstance(m, DepthwiseConvLayer)]
    assert blk.identity == (stride == 1 and inp == oup) and len(dws) == 1 and dws[0].kernel_size == k
    assert sum(isinstance(m, SELayer) for m in blk.modules()) == use_se and (blk.dw._gate is not None) == bool(use_se and inp != hidden)
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k_}": v for k_, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(inp)
    y = blk.fwd(to_nhwc(x, backend))
    assert_close(to_nchw_cpu(y), fx["y"], 2e-5, "training forward")
    dx = blk.bwd(to_nhwc(fx["dy"], backend))
    net.join_side()
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(blk, fx, 1e-4)
    for k_, b in blk.named_buffers():
        if not k_.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k_], 2e-5, k_)
    net.eval()
    with torch.no_grad():
        ye = to_nchw_cpu(blk.fwd(to_nhwc(x, backend)))
        assert_close(ye, fx["y_eval"], 2e-5, "eval forward")
        net.prep_model_for_conversion()
        assert blk.dw._folded is not None and blk.pwl._folded is not None
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend))), ye, 2e-5, "folded against unfolded eval forward")
    net.train()
    assert blk.dw._folded is None


# --------------------------------------------------------------------------------------------- models
def test_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import DepthwiseConvLayer, LinearLayer
    from super_gradients_amd.modules.se_blocks import SELayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.mobilenetv3 import InvertedResidual, MobileNetV3

    for name, last, n_dw, n_k5, n_se, exp in (("mobilenet_v3_large", 1280, 15, 6, 8, 960), ("mobilenet_v3_small", 1024, 11, 8, 9, 576)):
        net = models.get(name, num_classes=7)
        dws = [m for m in net.modules() if isinstance(m, DepthwiseConvLayer)]
        assert len(dws) == n_dw and sum(m.kernel_size == 5 for m in dws) == n_k5 and sum(isinstance(m, SELayer) for m in net.modules()) == n_se, name
        c0, c3 = net.classifier._modules["0"], net.classifier._modules["3"]
        assert net.last_channel == last and (c0.in_features, c0.out_features, c3.in_features, c3.out_features) == (exp, last, last, 7), name
        assert net.classifier._modules["2"].p == 0.2 and not list(net.classifier._modules["2"].state_dict())
        assert net.get_input_channels() == 3 and not net.supports_half_inference()
        assert net.gradient_buckets() == [f"features.{i}." for i in range(n_dw + 1)] + ["conv.", "classifier."]
    se = models.get("mobilenet_v3_large", num_classes=7).features._modules["4"].conv._modules["5"]
    assert se.fc._modules["0"].out_features == 24 and se.fc._modules["2"].in_features == 24  # _make_divisible(72 // 4, 8)
    assert models.get("mobilenet_v3_large", arch_params=dict(width_mult=1.25), num_classes=3).last_channel == 1600
    assert models.get("mobilenet_v3_small", arch_params=dict(width_mult=0.5), num_classes=3).last_channel == 1024
    net = models.get("mobilenet_v3_custom", arch_params=dict(width_mult=1.0, mode="small", structure=[[3, 1, 16, 1, 0, 2], [5, 4, 24, 1, 1, 1], [5, 3, 24, 0, 1, 1]],
                                                             in_channels=4), num_classes=3)
    blocks = [m for m in net.modules() if isinstance(m, InvertedResidual)]
    assert [(b.identity, b.stride) for b in blocks] == [(False, 2), (False, 1), (True, 1)] and net.last_channel == 1024 and net.get_input_channels() == 4
    net.replace_head(new_num_classes=5)
    head = net.classifier._modules["3"]
    assert isinstance(head, LinearLayer) and head.out_features == 5 and list(net.state_dict())[-2:] == ["classifier.3.weight", "classifier.3.bias"]
    assert net.get_finetune_lr_dict(0.1) == {"classifier": 0.1, "default": 0.0}
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=nn.Linear(1024, 2))
    with pytest.raises(ValueError):
        net.replace_head()
    # a 7x7 depthwise filter; an output width of 18 (divisor 8 gives 16 / 24: only a hand-built block can ask for it)
    with pytest.raises(NotImplementedError):
        MobileNetV3([[7, 1, 16, 0, 0, 1]], "small", num_classes=3)
    with pytest.raises(NotImplementedError):
        InvertedResidual(16, 64, 18, 3, 1, 0, 0)
    with pytest.raises(NotImplementedError):
        DepthwiseConvLayer(16, 1, kernel_size=7)


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_layout_matches_reference(name):
    from super_gradients_amd.training import models

    fx = _model_reference(name)
    net = models.get(name, num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["state_layout"]


@pytest.mark.parametrize("name", MODELS)
def test_checkpoint_round_trip_with_reference_live(name):
    """Both directions, strictly, against the reference's own model class (needs the reference tree)."""
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine (the recorded state layout is checked by test_state_dict_layout_matches_reference)")
    from super_gradients_amd.training import models

    ref_shim.install()
    import super_gradients.training.models.classification_models.mobilenetv3 as r
    from super_gradients.training.utils.utils import HpmStruct

    ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
    G.deterministic_fill(ref, seed=9)
    net = models.get(name, num_classes=10)
    net.load_state_dict(ref.state_dict(), strict=True)
    back = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
    back.load_state_dict(net.state_dict(), strict=True)
    for (k, a), b in zip(ref.state_dict().items(), back.state_dict().values()):
        assert torch.equal(a, b), k


def test_initial_weight_distributions():
    from super_gradients_amd.training import models

    sd = models.get("mobilenet_v3_large", num_classes=1000).state_dict()
    for key, k, out in (("conv.0.weight", 1, 960), ("features.15.conv.3.weight", 5, 960), ("features.0.0.weight", 3, 16)):
        std = float(sd[key].std())
        assert abs(std / (2.0 / (k * k * out)) ** 0.5 - 1.0) < 0.1, (key, std)
    for key in ("classifier.0", "classifier.3", "features.15.conv.5.fc.0"):
        assert abs(float(sd[key + ".weight"].std()) / 0.01 - 1.0) < 0.05 and float(sd[key + ".bias"].abs().max()) == 0.0
    assert bool((sd["features.5.conv.4.weight"] == 1).all()) and bool((sd["features.5.conv.4.bias"] == 0).all())


def _grad_check(norms, fx, what):
    """tests/test_resnet.py `_grad_check`."""
    t64, ref = fx["grad_norms_f64"], fx["grad_norms"]
    big = ref > 1e-3 * ref.max()
    e_hip = ((norms - t64).abs() / t64.clamp_min(1e-30))[big]
    e_ref = ((ref - t64).abs() / t64.clamp_min(1e-30))[big]
    msg = f"{what}: gradient norms vs fp64: worst {float(e_hip.max()):.2e} mean {float(e_hip.mean()):.2e}; reference fp32 worst {float(e_ref.max()):.2e} mean {float(e_ref.mean()):.2e}"
    print(msg)
    assert float(e_hip.max()) <= max(5e-3, 3.0 * float(e_ref.max())) and float(e_hip.mean()) <= max(1e-3, 3.0 * float(e_ref.mean())), msg


def _product_against_reference(name, device):
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    fx = _model_reference(name)
    net = models.get(name, num_classes=10)
    G.deterministic_fill(net, seed=4)
    net.classifier._modules["2"].p = 0.0
    net.materialize(device).train()
    x, y = _model_inputs()
    logits = net(x.to(device))
    loss = CrossEntropyLoss()(logits, y.to(device))
    loss.backward()
    e_pair = rel_err(logits.cpu(), fx["logits"])
    e_hip, e_cpu = rel_err(logits.cpu().double(), fx["logits_f64"]), rel_err(fx["logits"].double(), fx["logits_f64"])
    print(f"{name}: logits hip-ref32 {e_pair:.2e} hip-ref64 {e_hip:.2e} ref32-ref64 {e_cpu:.2e}; loss {float(loss.detach()):.6f} vs {float(fx['loss']):.6f}")
    assert e_pair <= 1e-4, f"training logits: hip-ref32 {e_pair:.2e} (hip-ref64 {e_hip:.2e}, ref32-ref64 {e_cpu:.2e})"
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-4 * abs(float(fx["loss"]))
    params = dict(net.named_parameters())
    _grad_check(torch.tensor([float(params[n].grad.double().norm()) for n in fx["grad_names"]], dtype=torch.float64), fx, name)
    for k, v in fx["bn_running_checksum"].items():
        assert abs(float(net.state_dict()[k].double().sum()) - v) <= 1e-4 * max(abs(v), 1.0), k
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))
    net.eval()
    with torch.no_grad():
        ev = net(x.to(device)).cpu()
        assert rel_err(ev, fx["eval_logits"]) <= 1e-4, f"eval logits {rel_err(ev, fx['eval_logits']):.2e}"
        net.prep_model_for_conversion()
        folded = net(x.to(device)).cpu()
    print(f"{name}: folded against unfolded eval logits {rel_err(folded, ev):.2e}")
    assert rel_err(folded, ev) <= 1e-4, f"prep_model_for_conversion changed the eval logits by {rel_err(folded, ev):.2e}"


@pytest.mark.parametrize("name", MODELS)
def test_product_mobilenetv3_emulation(name):
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference(name, torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_mobilenetv3_golden(gpu_device, name):
    _product_against_reference(name, gpu_device)


def test_custom_mobilenetv3_trains_with_dropout(backend):
    """mobilenet_v3_custom (three blocks: SE after the activation, SE between BatchNorm and hard-swish at 5x5, a 5x5 residual block) with the
    classifier's dropout at p = 0.2: training runs with finite non-zero gradients, two steps after the same torch.manual_seed give equal
    logits (another seed gives other logits), eval ignores p."""
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    arch = dict(width_mult=1.0, mode="small", structure=[[3, 1, 16, 1, 0, 2], [5, 4, 24, 1, 1, 1], [5, 3, 24, 0, 1, 1]])
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(4, 3, 16, 16, generator=g).to(backend), torch.randint(0, 3, (4,), generator=g).to(backend)
    torch.manual_seed(21)
    net = models.get("mobilenet_v3_custom", arch_params=dict(arch), num_classes=3)
    for k, p in net.named_parameters():  # (N(0, 0.01) linears give logits ~1e-4: widen them so that the dropped units show)
        if k.startswith("classifier") and k.endswith("weight"):
            p.data.mul_(30.0)
    assert net.classifier._modules["2"].p == 0.2
    net.materialize(backend).train()

    def step(seed):
        torch.manual_seed(seed)
        net.zero_grad()
        out = net(x)
        loss = CrossEntropyLoss()(out, y)
        loss.backward()
        return out.detach().cpu().clone(), loss.detach().cpu()

    a, loss = step(7)
    assert bool(torch.isfinite(loss))
    for k, p in net.named_parameters():
        gcpu = p.grad.cpu()
        assert bool(torch.isfinite(gcpu).all()) and float(gcpu.abs().max()) > 0, k
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    b, _ = step(8)
    net.load_state_dict(sd)  # (the running statistics moved; the training forward does not read them, this keeps eval below comparable)
    c, _ = step(7)
    assert torch.equal(a, c), "the same seed gives the same step"
    assert not torch.equal(a, b), "another seed drops other units"
    net.eval()
    with torch.no_grad():
        e1 = net(x).cpu()
        net.classifier._modules["2"].p = 0.9
        assert torch.equal(net(x).cpu(), e1), "eval ignores p"


# --------------------------------------------------------------------------------------------- trainer
def _train_params(epochs, **kw):
    return dict(max_epochs=epochs, lr_mode="CosineLRScheduler", initial_lr=0.05, cosine_final_lr_ratio=0, loss="CrossEntropyLoss", optimizer="SGD",
                optimizer_params=dict(momentum=0.9, weight_decay=1e-4), zero_weight_decay_on_bias_and_bn=True, average_best_models=False,
                metric_to_watch="Accuracy", greater_metric_to_watch_is_better=True, train_metrics_list=["Accuracy"], valid_metrics_list=["Accuracy"],
                silent_mode=True, seed=3, **kw)


@pytest.mark.gpu
def test_trainer_steps_mobilenet_v3_small(gpu_device, tmp_path):
    """Two Trainer steps (SGD, cross-entropy, dropout 0.2) of mobilenet_v3_small at 8 x 3 x 32 x 32: finite loss, the parameters move, every
    BatchNorm counted two batches."""
    from super_gradients_amd.training import Trainer, models

    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(8, 3, 32, 32, generator=g), torch.arange(8) % 6
    loader = [(x, labels)] * 2
    torch.manual_seed(11)
    net = models.get("mobilenet_v3_small", num_classes=6)
    before = {k: v.clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    res = Trainer("m3", ckpt_root_dir=str(tmp_path)).train(net, _train_params(1), loader, valid_loader=loader[:1])
    loss = res[-1]["train"]["CrossEntropyLoss"]
    assert loss == loss and abs(loss) < 1e4, res
    sd = net.state_dict()
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    moved = [k for k, v in before.items() if k.endswith("weight") and not torch.equal(v, sd[k].cpu())]
    assert len(moved) == sum(k.endswith("weight") for k in before), "parameters that did not change"
    assert all(bool(torch.isfinite(v.cpu()).all()) for v in sd.values() if v.dtype.is_floating_point)
