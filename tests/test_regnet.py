"""RegNet / AnyNet classifiers: the XBlock (grouped 3x3 convolution, squeeze-excitation with a hidden width that is padded inside, identity
and projection shortcuts), the registered models, the head's dropout and Trainer steps.

  reference (its own classification_models/regnet.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/regnet_*.pt elsewhere (tests/make_regnet_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars as tests/test_mobilenetv3.py.  A block: forward output, running statistics and eval output at 2e-5, input and parameter gradients at
1e-4 (relative, max-norm).  A whole model: logits and loss at 1e-4, parameter gradients by tests/test_resnet.py's `_grad_check`.  On this
input (4 x 3 x 64 x 64, seed 5) the reference's own fp32 run is, against its fp64 run (tests/make_regnet_golden.py prints it): logits
4.4e-6 (regnetY200) / 1.3e-5 (regnetY800), per-parameter gradient norms overall 9.7e-4 / 3.1e-5 - inside a third of the 1e-4 bar.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc

MODELS = ["regnetY200", "regnetY800"]
CLS = {"regnetY200": "RegNetY200", "regnetY800": "RegNetY800"}
# (in_channels, out_channels, bottleneck_ratio, group_width, stride, se_ratio): no SE, identity shortcut (cg 8, 3 groups); SE, identity
# shortcut, hidden width 24 // 4 = 6 (padded to 8 inside); SE at stride 2 with a projection shortcut (hidden 8, cg 16, 4 groups); no SE,
# stride 2 projection with an odd group count (cg 8, 5 groups)
BLOCKS = {"plain_id": (24, 24, 1, 8, 1, None), "se_id_pad": (24, 24, 1, 8, 1, 4), "se_s2_proj": (32, 64, 1, 16, 2, 4), "plain_s2_proj": (24, 40, 1, 8, 2, None)}
ANYNET = dict(ls_num_blocks=[1, 2], ls_block_width=[24, 48], ls_bottleneck_ratio=[1, 1], ls_group_width=[8, 8], stride=2, se_ratio=4)


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
        from super_gradients.training.models.classification_models.regnet import XBlock as RefBlock

        out = {}
        for i, (name, cfg) in enumerate(BLOCKS.items()):
            torch.manual_seed(7 + i)
            blk = RefBlock(*cfg)
            G.deterministic_fill(blk, seed=11 + i)
            out[name] = _record_step(blk, _block_input(cfg[0]), 5 + i)
        return out

    return G.reference_outputs("regnet_block_reference", compute)


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)


def _model_reference(name):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.regnet as r
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

    return G.reference_outputs(f"regnet_{name}_reference", compute)


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
def test_xblock_against_reference(backend, cfg):
    """The product block against the reference's XBlock: training forward, input gradient, every parameter gradient (the grouped filter and the
    SE convolutions in the reference's shapes included), running statistics after the step, eval forward, the folded eval form."""
    from super_gradients_amd.modules.layers import GroupedConvLayer
    from super_gradients_amd.training.models.classification_models.regnet import SqueezeExcite, XBlock

    cin, cout, br, gw, stride, se_ratio = BLOCKS[cfg]
    fx = _block_reference()[cfg]
    blk = XBlock(*BLOCKS[cfg])
    assert list(blk.state_dict().keys()) == list(fx["state"].keys())
    assert [tuple(v.shape) for v in blk.state_dict().values()] == [tuple(v.shape) for v in fx["state"].values()]
    gl = [m for m in blk.modules() if isinstance(m, GroupedConvLayer)]
    assert len(gl) == 1 and gl[0].groups == cout // gw and gl[0].stride == stride and tuple(gl[0].weight.shape) == (cout, gw, 3, 3)
    ses = [m for m in blk.modules() if isinstance(m, SqueezeExcite)]
    assert len(ses) == (se_ratio is not None) and (blk.shortcut is not None) == (stride != 1 or cin != cout)
    if ses:
        assert ses[0].hidden == cin // se_ratio and ses[0]._hp % 4 == 0 and (cfg != "se_id_pad" or (ses[0].hidden, ses[0]._hp) == (6, 8))
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k_}": v for k_, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(cin)
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
        assert blk.conv_block_2._folded is not None and blk.conv_block_3._folded is not None
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend))), ye, 2e-5, "folded against unfolded eval forward")
    net.train()
    assert blk.conv_block_2._folded is None


# --------------------------------------------------------------------------------------------- models
def test_conv_layer_routing():
    """1 < groups < channels with a 3x3 pad-1 filter and a built width goes to the grouped layer; every other grouped request keeps its refusal."""
    from super_gradients_amd.modules.conv_bn_act_block import _conv_layer
    from super_gradients_amd.modules.layers import ConvLayer, DepthwiseConvLayer, GroupedConvLayer

    assert isinstance(_conv_layer(64, 64, 3, 2, 1, 4), GroupedConvLayer) and isinstance(_conv_layer(152, 152, 3, 1, 1, 19), GroupedConvLayer)
    assert isinstance(_conv_layer(64, 64, 3, 1, 1, 64), DepthwiseConvLayer) and isinstance(_conv_layer(64, 64, 3, 1, 1, 1), ConvLayer)
    for args in ((64, 64, 3, 1, 1, 32), (64, 128, 3, 1, 1, 4), (64, 64, 5, 1, 2, 4), (64, 64, 3, 1, 0, 4), (64, 64, 1, 1, 0, 4), (96, 96, 3, 1, 1, 8), (64, 64, 3, 3, 1, 4)):
        with pytest.raises(NotImplementedError, match="4, 8, 16, 32, 64"):
            _conv_layer(*args)


def test_parameter_arithmetic_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import GroupedConvLayer, LinearLayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.regnet import (AnyNetX, SqueezeExcite, XBlock, regnet_params_to_blocks,
                                                                                  verify_correctness_of_parameters)

    table = {"regnetY200": ((24, 36, 2.5, 13, 1, 8), [1, 1, 4, 7], [24, 64, 152, 376], 8), "regnetY400": ((48, 28, 2.1, 16, 1, 8), [1, 3, 6, 6], [48, 104, 208, 448], 8),
             "regnetY600": ((48, 33, 2.3, 15, 1, 16), [1, 3, 7, 4], [48, 112, 256, 576], 16), "regnetY800": ((56, 39, 2.4, 14, 1, 16), [1, 3, 8, 2], [64, 128, 320, 768], 16)}
    for name, (params, nblocks, _, gw) in table.items():
        nb, widths, ratios, gws = regnet_params_to_blocks(*params)
        assert list(nb) == nblocks and set(gws) == {gw} and set(ratios) == {1} and all(w % gw == 0 for w in widths), name
        net = models.get(name, num_classes=7)
        assert net.ls_block_width == widths and [len(st.blocks.children_list()) for k, st in net.net._modules.items() if k.startswith("stage_")] == nblocks
        gl = [m for m in net.modules() if isinstance(m, GroupedConvLayer)]
        assert len(gl) == sum(nblocks) and all(m.in_channels // m.groups == gw for m in gl), name
        assert sum(isinstance(m, SqueezeExcite) for m in net.modules()) == sum(nblocks)
        assert net.get_input_channels() == 3 and not net.supports_half_inference() and net.net.head.fc.out_features == 7
        assert net.gradient_buckets() == ["net.stem."] + [f"net.stage_{i}." for i in range(4)] + ["net.head."]
    with pytest.raises(AssertionError):
        verify_correctness_of_parameters([1, 2], [48, 24], [1, 1], [8, 8])
    with pytest.raises(AssertionError):
        verify_correctness_of_parameters([1, 2], [24, 48], [1, 1], [8, 16])
    net = models.get("regnetY200", arch_params=dict(dropout_prob=0.5), num_classes=7)
    assert net.net.head.dropout.p == 0.5 and not list(net.net.head.dropout.state_dict())
    se = net.net.stage_1.blocks.block_0.se
    assert (se.hidden, se._hp) == (6, 8) and tuple(se._modules["1"].weight.shape) == (6, net.ls_block_width[1], 1, 1)
    net.replace_head(new_num_classes=5)
    assert isinstance(net.net.head.fc, LinearLayer) and net.net.head.fc.out_features == 5 and list(net.state_dict())[-2:] == ["net.head.fc.weight", "net.head.fc.bias"]
    assert net.net.head.dropout.p == 0.5 and net.get_finetune_lr_dict(0.1) == {"net.head": 0.1, "default": 0}
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=nn.Linear(376, 2))
    with pytest.raises(ValueError):
        net.replace_head()
    net.replace_input_channels(5)
    assert net.get_input_channels() == 5 and tuple(net.state_dict()["net.stem.conv.weight"].shape) == (32, 5, 3, 3)
    nas = models.get("nas_regnet", arch_params=dict(structure=[24, 36, 2.5, 13, 1, 8, 2, 0]), num_classes=3)
    assert not any(isinstance(m, SqueezeExcite) for m in nas.modules()) and nas.ls_block_width == table["regnetY200"][2]
    cust = models.get("custom_regnet", arch_params=dict(initial_width=24, slope=36, quantized_param=2.5, network_depth=13, bottleneck_ratio=1, group_width=8, stride=2,
                                                        se_ratio=4, input_channels=4), num_classes=3)
    assert cust.get_input_channels() == 4 and any(isinstance(m, SqueezeExcite) for m in cust.modules())
    with pytest.raises(NotImplementedError, match="DropPath"):
        models.get("regnetY200", arch_params=dict(droppath_prob=0.1), num_classes=3)
    with pytest.raises(NotImplementedError, match="DropPath"):
        XBlock(24, 24, 1, 8, 1, 4, droppath_prob=0.2)
    with pytest.raises(NotImplementedError, match="4, 8, 16, 32, 64"):  # 12 channels per group
        AnyNetX([1], [24], [1], [12], 2, 3, None, False)


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_layout_matches_reference(name):
    from super_gradients_amd.training import models

    fx = _model_reference(name)
    net = models.get(name, num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["state_layout"]


@pytest.mark.parametrize("name", MODELS)
def test_checkpoint_round_trip_through_the_reference_key_names(name):
    """A state_dict with the reference's key names and shapes loads strictly and comes back bit for bit (the grouped filters through their
    arena layout once the model is materialised on the host emulation)."""
    import emu_env
    from super_gradients_amd.training import models

    fx = _model_reference(name)
    g = torch.Generator().manual_seed(9)
    sd = {k: (torch.randn(shape, generator=g) if "num_batches_tracked" not in k else torch.tensor(3)) for k, shape in fx["state_layout"]}
    net = models.get(name, num_classes=10)
    net.load_state_dict(sd, strict=True)
    emu_env.activate()
    try:
        net.materialize(torch.device("cpu"))
        back = net.state_dict()
    finally:
        emu_env.deactivate()
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v), k


def test_initial_weight_distributions():
    from super_gradients_amd.training import models

    sd = models.get("regnetY800", num_classes=1000).state_dict()
    for key, k, out in (("net.stem.conv.weight", 3, 32), ("net.stage_3.blocks.block_0.conv_block_2.0.weight", 3, 768), ("net.stage_2.blocks.block_1.conv_block_1.0.weight", 1, 320),
                        ("net.stage_3.blocks.block_1.se.3.weight", 1, 768)):
        std = float(sd[key].std())
        assert abs(std / (2.0 / (k * k * out)) ** 0.5 - 1.0) < 0.1, (key, std)
    assert abs(float(sd["net.head.fc.weight"].std()) / 0.01 - 1.0) < 0.05 and float(sd["net.head.fc.bias"].abs().max()) == 0.0
    assert bool((sd["net.stage_1.blocks.block_0.conv_block_2.1.weight"] == 1).all()) and bool((sd["net.stage_1.blocks.block_0.conv_block_2.1.bias"] == 0).all())


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


def test_product_regnetY200_emulation():
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference("regnetY200", torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_regnet_golden(gpu_device, name):
    _product_against_reference(name, gpu_device)


def test_custom_anynet_backbone_mode(backend):
    """custom_anynet without its head: the NCHW feature map of the last stage, and a backward pass from a gradient of that shape."""
    from super_gradients_amd.training import models

    torch.manual_seed(3)
    net = models.get("custom_anynet", arch_params=dict(ANYNET, backbone_mode=True), num_classes=3)
    assert "head" not in net.net._modules and not any(k.startswith("net.head") for k in net.state_dict())
    net.materialize(backend).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(backend)
    y = net(x)
    assert tuple(y.shape) == (2, 48, 4, 4) and bool(torch.isfinite(y).all()) and float(y.min()) >= 0.0
    net.zero_grad()
    y.backward(torch.ones_like(y))
    g = dict(net.named_parameters())["net.stage_1.blocks.block_1.conv_block_2.0.weight"].grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_custom_anynet_trains_with_dropout(backend):
    """The head's dropout at p = 0.5 (the recipe's value): finite non-zero gradients, two steps after the same torch.manual_seed give equal
    logits (another seed gives other logits), eval ignores p."""
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(4, 3, 32, 32, generator=g).to(backend), torch.randint(0, 3, (4,), generator=g).to(backend)
    torch.manual_seed(21)
    net = models.get("custom_anynet", arch_params=dict(ANYNET, dropout_prob=0.5), num_classes=3)
    net.net.head.fc.weight.data.mul_(30.0)  # (N(0, 0.01) gives logits ~1e-3: widen it so that the dropped units show)
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
    grads = [p.grad for p in net.parameters()]
    assert all(bool(torch.isfinite(gr).all()) for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)
    b, _ = step(7)
    c, _ = step(8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    net.eval()
    with torch.no_grad():
        e1, e2 = net(x).cpu(), net(x).cpu()
    assert torch.equal(e1, e2)
    net.net.head.dropout.p = 0.0
    net.train()
    d, _ = step(7)
    assert not torch.equal(a, d)


# --------------------------------------------------------------------------------------------- trainer
@pytest.mark.gpu
def test_trainer_steps_regnetY200_rmsprop_tf_ema(gpu_device, tmp_path):
    """Two Trainer steps of regnetY200 at 8 x 3 x 32 x 32 with the optimizer and averaging of recipes/imagenet_regnetY.yaml (RMSpropTF, constant-decay
    EMA, StepLRScheduler, label smoothing, dropout 0.5): finite loss, the parameters move, every BatchNorm counted two batches."""
    from super_gradients_amd.training import Trainer, models

    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(8, 3, 32, 32, generator=g), torch.arange(8) % 6
    loader = [(x, labels)] * 2
    torch.manual_seed(11)
    net = models.get("regnetY200", arch_params=dict(dropout_prob=0.5), num_classes=6)
    before = {k: v.clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    tp = dict(max_epochs=1, lr_mode="StepLRScheduler", step_lr_update_freq=2.4, lr_decay_factor=0.97, initial_lr=0.016, loss="CrossEntropyLoss", criterion_params=dict(smooth_eps=0.1),
              optimizer="RMSpropTF", optimizer_params=dict(weight_decay=4e-5, alpha=0.9, momentum=0.9, eps=0.001), zero_weight_decay_on_bias_and_bn=True,
              ema=True, ema_params=dict(decay=0.9999, decay_type="constant"), average_best_models=False, metric_to_watch="Accuracy",
              greater_metric_to_watch_is_better=True, train_metrics_list=["Accuracy"], valid_metrics_list=["Accuracy"], silent_mode=True, seed=3)
    res = Trainer("regnet", ckpt_root_dir=str(tmp_path)).train(net, tp, loader, valid_loader=loader[:1])
    loss = res[-1]["train"]["CrossEntropyLoss"]
    assert loss == loss and abs(loss) < 1e4, res
    sd = net.state_dict()
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    moved = [k for k, v in before.items() if k.endswith("weight") and not torch.equal(v, sd[k].cpu())]
    assert len(moved) == sum(k.endswith("weight") for k in before), "parameters that did not change"
    assert all(bool(torch.isfinite(v.cpu()).all()) for v in sd.values() if v.dtype.is_floating_point)
