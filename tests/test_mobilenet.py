"""MobileNetV2 classifiers: the inverted-residual block (1x1 expand, depthwise 3x3, 1x1 project; ReLU6), the mobilenet_v2 models and Trainer steps.

  reference (its own classification_models/mobilenetv2.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/mobilenet_*.pt elsewhere (tests/make_mobilenet_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars.  A block: tests/test_blocks.py's `_check` - forward output, running statistics and eval output at 2e-5, input and parameter gradients at
1e-4 (relative, max-norm).  A whole model: logits and loss at 1e-4 as tests/test_resnet.py and tests/test_repvgg.py; parameter gradients by
tests/test_resnet.py's `_grad_check` (per-parameter norms against the fp64 run of the same modules, no further from it than 3 x the
reference's own fp32 run).  On this input the reference's own fp32 run is, against its fp64 run (tests/make_mobilenet_golden.py prints it):
per-parameter gradient NORMS 5.2e-4 (mobilenet_v2) / 7.6e-4 (mobile_net_v2_135) overall; gradient ELEMENTS differ at the per-cent level
(ReLU6 flips and 2 x 2 maps at batch 4), so an element-wise whole-model comparison is meaningless and none is made.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc

MODELS = ["mobilenet_v2", "mobile_net_v2_135"]
CLS = {"mobilenet_v2": "MobileNetV2Base", "mobile_net_v2_135": "MobileNetV2_135"}
# (inp, oup, stride, expand_ratio): with residual; stride 2; the t == 1 form (depthwise first); t == 1 with residual (its gradient joins the
# depthwise data gradient)
BLOCKS = {"res": (16, 16, 1, 6), "s2": (16, 24, 2, 6), "t1": (32, 16, 1, 1), "t1res": (16, 16, 1, 1)}


# --------------------------------------------------------------------------------------------- reference side (recorded tensors)
def _block_input(c):
    return torch.randn(2, c, 6, 6, generator=torch.Generator().manual_seed(1)) + 0.5


def _record_step(mod, x, seed):
    """One training step (a seeded upstream gradient) and the eval forward after it, of a reference module (tests/test_repvgg.py's scheme)."""
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
        from super_gradients.training.models.classification_models.mobilenetv2 import InvertedResidual as RefBlock

        out = {}
        for i, (name, (inp, oup, stride, t)) in enumerate(BLOCKS.items()):
            torch.manual_seed(7 + i)
            blk = RefBlock(inp, oup, stride, expand_ratio=t)
            G.deterministic_fill(blk, seed=11 + i)
            out[name] = _record_step(blk, _block_input(inp), 5 + i)
        return out

    return G.reference_outputs("mobilenet_block_reference", compute)


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)


def _model_reference(name):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.mobilenetv2 as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
        G.deterministic_fill(ref, seed=4)
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

    return G.reference_outputs(f"mobilenet_{name}_reference", compute)


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
    """tests/test_blocks.py `_check`: every parameter gradient, relative to its own largest element with a floor of 1 % of the largest of all."""
    gmax = max(float(g.abs().max()) for g in fx["grads"].values())
    for name, p in net.named_parameters():
        rg = fx["grads"][name]
        e = float((p.grad.cpu().double().reshape(rg.shape) - rg.double()).abs().max()) / max(float(rg.abs().max()), 1e-2 * gmax)
        assert e <= tol, f"grad {name}: {e:.3e}"


@pytest.mark.parametrize("cfg", list(BLOCKS))
def test_inverted_residual_against_reference(backend, cfg):
    """The product block against the reference's InvertedResidual: training forward, input gradient, every parameter gradient (the depthwise
    filter's included), running statistics after the step, eval forward, and the folded eval form against the unfolded one."""
    from super_gradients_amd.modules.layers import DepthwiseConvLayer
    from super_gradients_amd.training.models.classification_models.mobilenetv2 import InvertedResidual

    inp, oup, stride, t = BLOCKS[cfg]
    fx = _block_reference()[cfg]
    blk = InvertedResidual(inp, oup, stride, expand_ratio=t)
    assert list(blk.state_dict().keys()) == list(fx["state"].keys())
    assert [tuple(v.shape) for v in blk.state_dict().values()] == [tuple(v.shape) for v in fx["state"].values()]
    assert blk.use_res_connect == (cfg in ("res", "t1res")) and sum(isinstance(m, DepthwiseConvLayer) for m in blk.modules()) == 1
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k}": v for k, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(inp)
    y = blk.fwd(to_nhwc(x, backend))
    assert_close(to_nchw_cpu(y), fx["y"], 2e-5, "training forward")
    dx = blk.bwd(to_nhwc(fx["dy"], backend))
    net.join_side()
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(blk, fx, 1e-4)
    for k, b in blk.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 2e-5, k)
    net.eval()
    with torch.no_grad():
        ye = to_nchw_cpu(blk.fwd(to_nhwc(x, backend)))
        assert_close(ye, fx["y_eval"], 2e-5, "eval forward")
        net.prep_model_for_conversion()
        assert blk.dw._folded is not None and blk.pwl._folded is not None
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend))), ye, 2e-5, "folded against unfolded eval forward")
    net.train()
    assert blk.dw._folded is None  # a training step follows: the folded copies are dropped


# --------------------------------------------------------------------------------------------- models
def test_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import DepthwiseConvLayer, LinearLayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.mobilenetv2 import InvertedResidual, MobileNetV2

    for name, last, widest in (("mobilenet_v2", 1280, 960), ("mobile_net_v2_135", 1728, 1296)):
        net = models.get(name, num_classes=7)
        assert len(net.state_dict()) == 314, name
        dws = [m for m in net.modules() if isinstance(m, DepthwiseConvLayer)]
        assert len(dws) == 17 and max(m.in_channels for m in dws) == widest and {m.stride for m in dws} == {1, 2}, name
        head = net.classifier._modules["1"]
        assert net.last_channel == last and head.in_features == last and head.out_features == 7, name
        assert net.get_input_channels() == 3 and not net.supports_half_inference()
        assert net.features._modules["1"].conv._modules["3"].out_channels == 16  # the t == 1 stage is not scaled by width_mult
    net = models.get("custom_mobilenet_v2", arch_params=dict(width_mult=0.5, structure=[[1, 16, 1, 1], [6, 24, 2, 2]], in_channels=4, dropout=0.1), num_classes=3)
    blocks = [m for m in net.modules() if isinstance(m, InvertedResidual)]
    assert [(b.use_res_connect, b.stride) for b in blocks] == [(False, 1), (False, 2), (True, 1)]
    assert blocks[1].conv._modules["6"].out_channels == 16 and net.last_channel == 1280 and net.get_input_channels() == 4  # make_divisible(24 * 0.5) = 16
    net.replace_head(new_num_classes=5)
    head = net.classifier._modules["1"]
    assert isinstance(head, LinearLayer) and head.out_features == 5 and list(net.state_dict())[-2:] == ["classifier.1.weight", "classifier.1.bias"]
    assert net.get_finetune_lr_dict(0.1) == {"classifier": 0.1, "default": 0.0}
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=nn.Linear(1280, 2))
    with pytest.raises(ValueError):
        net.replace_head()
    # backbone mode; grouped (not depthwise) convolutions; a stage width of 18; a hidden width of int(16 * 1.125) = 18
    for bad in (dict(backbone_mode=True), dict(grouped_conv_size=2), dict(structure=[[1, 18, 1, 1]]), dict(structure=[[1, 16, 1, 1], [1.125, 24, 1, 1]])):
        with pytest.raises(NotImplementedError):
            MobileNetV2(num_classes=3, dropout=0.0, **bad)


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
    import super_gradients.training.models.classification_models.mobilenetv2 as r
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
    """_initialize_weights as the reference's: conv N(0, sqrt(2 / (k k out))), BatchNorm 1 / 0, linear N(0, 0.01) with zero bias."""
    from super_gradients_amd.training import models

    net = models.get("mobilenet_v2", num_classes=1000)
    sd = net.state_dict()
    for key, k, out in (("features.18.0.weight", 1, 1280), ("features.17.conv.3.weight", 3, 960), ("features.0.0.weight", 3, 32)):
        std = float(sd[key].std())
        assert abs(std / (2.0 / (k * k * out)) ** 0.5 - 1.0) < 0.1, (key, std)
    assert abs(float(sd["classifier.1.weight"].std()) / 0.01 - 1.0) < 0.05 and float(sd["classifier.1.bias"].abs().max()) == 0.0
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
def test_product_mobilenet_emulation(name):
    """The whole model on the host emulation of the kernels (CPU tensors): logits, loss, gradient norms, running statistics, eval, folded eval."""
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference(name, torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_mobilenet_golden(gpu_device, name):
    _product_against_reference(name, gpu_device)


def test_custom_mobilenet_trains_and_dropout_is_refused_in_training(backend):
    """custom_mobilenet_v2 with a two-stage structure at width_mult 0.5 (its second stage holds a residual block): a training step against
    autograd over the same arithmetic is the block tests' job - here the model runs, its gradients are finite and non-zero, eval works with
    dropout > 0 (the identity) and training with dropout > 0 raises."""
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    arch = dict(width_mult=0.5, structure=[[1, 16, 1, 1], [6, 24, 2, 2]])
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(4, 3, 16, 16, generator=g).to(backend), torch.randint(0, 3, (4,), generator=g).to(backend)
    net = models.get("custom_mobilenet_v2", arch_params=dict(arch), num_classes=3)
    net.materialize(backend).train()
    loss = CrossEntropyLoss()(net(x), y)
    loss.backward()
    assert bool(torch.isfinite(loss.detach().cpu()))
    for k, p in net.named_parameters():
        gcpu = p.grad.cpu()
        assert bool(torch.isfinite(gcpu).all()) and float(gcpu.abs().max()) > 0, k
    drop = models.get("custom_mobilenet_v2", arch_params=dict(arch, dropout=0.2), num_classes=3)
    drop.materialize(backend).eval()
    with torch.no_grad():
        assert tuple(drop(x).shape) == (4, 3)
    drop.train()
    with pytest.raises(NotImplementedError):
        drop(x)


# --------------------------------------------------------------------------------------------- trainer
def _train_params(epochs, **kw):
    return dict(max_epochs=epochs, lr_mode="CosineLRScheduler", initial_lr=0.05, cosine_final_lr_ratio=0, loss="CrossEntropyLoss", optimizer="SGD",
                optimizer_params=dict(momentum=0.9, weight_decay=1e-4), zero_weight_decay_on_bias_and_bn=True, average_best_models=False,
                metric_to_watch="Accuracy", greater_metric_to_watch_is_better=True, train_metrics_list=["Accuracy"], valid_metrics_list=["Accuracy"],
                silent_mode=True, seed=3, **kw)


@pytest.mark.gpu
def test_trainer_steps_mobilenet_v2(gpu_device, tmp_path):
    """Three Trainer steps (SGD, cross-entropy) of mobilenet_v2 at 8 x 3 x 32 x 32: finite loss, the parameters move, every BatchNorm counted
    three batches; then one hand-driven step with ArenaAdamW and ModelEMA."""
    from super_gradients_amd.training import Trainer, models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.ema import ModelEMA
    from super_gradients_amd.training.utils.optimizers import ArenaAdamW

    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(8, 3, 32, 32, generator=g), torch.arange(8) % 6
    loader = [(x, labels)] * 3
    torch.manual_seed(11)
    net = models.get("mobilenet_v2", num_classes=6)
    before = {k: v.clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    res = Trainer("m", ckpt_root_dir=str(tmp_path)).train(net, _train_params(1), loader, valid_loader=loader[:1])
    loss = res[-1]["train"]["CrossEntropyLoss"]
    assert loss == loss and abs(loss) < 1e4, res
    sd = net.state_dict()
    assert all(int(v) == 3 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    moved = [k for k, v in before.items() if k.endswith("weight") and not torch.equal(v, sd[k].cpu())]
    assert len(moved) == sum(k.endswith("weight") for k in before), "parameters that did not change"
    assert all(bool(torch.isfinite(v.cpu()).all()) for v in sd.values() if v.dtype.is_floating_point)
    # one step with the arena AdamW and the EMA of the weights
    net.train()
    opt = ArenaAdamW(net, lr=1e-3, weight_decay=1e-5, zero_weight_decay_on_bias_and_bn=True)
    ema = ModelEMA.from_params(net, decay=0.9, decay_type="constant")
    w0 = net.p_arena.buf.clone()
    out = net(x.to(gpu_device))
    CrossEntropyLoss()(out, labels.to(gpu_device)).backward()
    opt.step()
    opt.zero_grad()
    ema.update(net, step=0, total_steps=10)
    assert not torch.equal(w0, net.p_arena.buf) and bool(torch.isfinite(net.p_arena.buf).all())
    assert bool(torch.isfinite(ema.p_ema).all()) and not torch.equal(ema.p_ema, w0) and not torch.equal(ema.p_ema, net.p_arena.buf)
