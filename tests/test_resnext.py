"""ResNeXt classifiers: the ResNet bottleneck with a grouped 3x3 conv2 (csrc/gconv.h through GroupedConvLayer).

  reference (its own classification_models/resnext.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/resnext_*.pt elsewhere (tests/make_resnext_golden.py writes them)
  product (HIP kernels; the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars as tests/test_regnet.py: resnext50's logits and loss at 1e-4, parameter gradients by tests/test_resnet.py's `_grad_check`, running
statistics, eval logits and the folded eval form.  resnext101: state layout and one forward.  On this input (4 x 3 x 96 x 96, seed 5) the
reference's own fp32 logits are 2.2e-5 (resnext50) from its fp64 logits - inside a third of the 1e-4 bar; at 64 x 64 they were 3.9e-5, outside it (tests/make_resnext_golden.py prints it).
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import rel_err

CLS = {"resnext50": "ResNeXt50", "resnext101": "ResNeXt101"}


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 96, 96, generator=g), torch.randint(0, 10, (4,), generator=g)


def _model_reference(name):
    """resnext50: one training step and the eval forward; resnext101: the state layout and the eval forward only (a small fixture)."""

    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.resnext as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
        G.deterministic_fill(ref, seed=4)
        layout = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        x, y = _model_inputs()
        out = dict(state_layout=layout)
        if name == "resnext50":
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
            out.update(logits=logits.detach(), loss=loss.detach(), logits_f64=logits64.detach(), grad_names=names,
                       grad_norms=torch.tensor([float(p32[k].grad.double().norm()) for k in names], dtype=torch.float64),
                       grad_norms_f64=torch.tensor([float(p64[k].grad.norm()) for k in names], dtype=torch.float64),
                       bn_running_checksum={k: float(v.double().sum()) for k, v in ref.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")})
        ref.eval()
        with torch.no_grad():
            out["eval_logits"] = ref(x)
        return out

    return G.reference_outputs(f"resnext_{name}_reference", compute)


def test_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import GroupedConvLayer, LinearLayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.resnext import GroupedConvBlock, ResNeXt

    for name, nblocks, cgs in (("resnext50", [3, 4, 6, 3], [4, 8, 16, 32]), ("resnext101", [3, 4, 23, 3], [8, 16, 32, 64])):
        net = models.get(name, num_classes=7)
        gl = [m for m in net.modules() if isinstance(m, GroupedConvLayer)]
        assert len(gl) == sum(nblocks) and all(m.groups == 32 for m in gl), name
        assert [getattr(net, f"layer{i + 1}").blocks()[0].conv2.in_channels // 32 for i in range(4)] == cgs, name
        assert [getattr(net, f"layer{i + 1}").blocks()[0].conv2.stride for i in range(4)] == [1, 2, 2, 2]
        assert [len(getattr(net, f"layer{i + 1}").blocks()) for i in range(4)] == nblocks
        assert net.get_input_channels() == 3 and net.fc.out_features == 7 and net.gradient_buckets()[-1] == "fc."
        assert len(net.layer1.blocks()[0].downsample) == 2 and len(net.layer1.blocks()[1].downsample) == 0
    net = models.get("resnext50", num_classes=7)
    net.replace_head(new_num_classes=5)
    assert isinstance(net.fc, LinearLayer) and net.fc.out_features == 5 and list(net.state_dict())[-2:] == ["fc.weight", "fc.bias"]
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=nn.Linear(2048, 2))
    net.replace_input_channels(4)
    assert net.get_input_channels() == 4 and tuple(net.state_dict()["conv1.weight"].shape) == (64, 4, 7, 7)
    with pytest.raises(NotImplementedError, match="dilat"):
        ResNeXt([3, 4, 6, 3], 32, 4, replace_stride_with_dilation=[False, True, False])
    with pytest.raises(ValueError):
        ResNeXt([3, 4, 6, 3], 32, 4, replace_stride_with_dilation=[False, True])
    with pytest.raises(NotImplementedError, match="dilat"):
        GroupedConvBlock(64, 64, groups=32, base_width=4, dilation=2)


@pytest.mark.parametrize("name", list(CLS))
def test_state_dict_layout_matches_reference(name):
    from super_gradients_amd.training import models

    fx = _model_reference(name)
    net = models.get(name, num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["state_layout"]
    assert dict(fx["state_layout"])["layer1.0.conv2.weight"] == ((128, 4, 3, 3) if name == "resnext50" else (256, 8, 3, 3))


def test_checkpoint_round_trip_through_the_reference_key_names():
    """A state_dict with the reference's key names and shapes loads strictly and comes back bit for bit from the materialised model."""
    import emu_env
    from super_gradients_amd.training import models

    fx = _model_reference("resnext50")
    g = torch.Generator().manual_seed(9)
    sd = {k: (torch.randn(shape, generator=g) if "num_batches_tracked" not in k else torch.tensor(3)) for k, shape in fx["state_layout"]}
    net = models.get("resnext50", num_classes=10)
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


def _grad_check(norms, fx, what):
    """tests/test_resnet.py `_grad_check`."""
    t64, ref = fx["grad_norms_f64"], fx["grad_norms"]
    big = ref > 1e-3 * ref.max()
    e_hip = ((norms - t64).abs() / t64.clamp_min(1e-30))[big]
    e_ref = ((ref - t64).abs() / t64.clamp_min(1e-30))[big]
    msg = f"{what}: gradient norms vs fp64: worst {float(e_hip.max()):.2e} mean {float(e_hip.mean()):.2e}; reference fp32 worst {float(e_ref.max()):.2e} mean {float(e_ref.mean()):.2e}"
    print(msg)
    assert float(e_hip.max()) <= max(5e-3, 3.0 * float(e_ref.max())) and float(e_hip.mean()) <= max(1e-3, 3.0 * float(e_ref.mean())), msg


def _folded_eval(net, x, ev):
    from super_gradients_amd.training.models.classification_models.resnext import GroupedConvBlock

    net.prep_model_for_conversion()
    blocks = [m for m in net.modules() if isinstance(m, GroupedConvBlock)]
    assert all(b._folded is not None and 1 in b._folded for b in blocks)
    folded = net(x).cpu()
    print(f"folded against unfolded eval logits {rel_err(folded, ev):.2e}")
    assert rel_err(folded, ev) <= 1e-4, f"prep_model_for_conversion changed the eval logits by {rel_err(folded, ev):.2e}"
    net.train()
    assert all(b._folded is None for b in blocks)


def _product_against_reference(device):
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    name = "resnext50"
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
        _folded_eval(net, x.to(device), ev)


@pytest.mark.gpu
def test_product_resnext50_golden(gpu_device):
    _product_against_reference(gpu_device)


@pytest.mark.gpu
def test_product_resnext101_forward_golden(gpu_device):
    from super_gradients_amd.training import models

    fx = _model_reference("resnext101")
    net = models.get("resnext101", num_classes=10)
    G.deterministic_fill(net, seed=4)
    net.materialize(gpu_device).eval()
    x, _ = _model_inputs()
    with torch.no_grad():
        ev = net(x.to(gpu_device)).cpu()
    assert rel_err(ev, fx["eval_logits"]) <= 1e-4, f"eval logits {rel_err(ev, fx['eval_logits']):.2e}"


def test_small_resnext_trains_on_the_emulation():
    """A two-block-per-layer ResNeXt (cardinality 4: 4 / 8 / 16 / 32 channels per group as resnext50) against the same network in torch on
    the host emulation: training logits at 1e-4, parameter gradient norms by `_grad_check` (torch's own fp32 run is the yardstick), the folded eval form."""
    import emu_env
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.models.classification_models.resnext import ResNeXt

    torch.manual_seed(5)
    net = ResNeXt([1, 1, 1, 1], 4, 4, num_classes=5)
    G.deterministic_fill(net, seed=6)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 5, (4,), generator=g)

    def conv(inp, w, stride=1, pad=0, groups=1):
        return F.conv2d(inp, w, None, stride, pad, 1, groups)

    def torch_step(dtype):
        ps = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}

        def bn(inp, p):
            return F.batch_norm(inp, None, None, ps[p + ".weight"], ps[p + ".bias"], True, 0.1, 1e-5)

        a = F.max_pool2d(F.relu(bn(conv(x.to(dtype), ps["conv1.weight"], 2, 3), "bn1")), 3, 2, 1)
        for i, stride in enumerate([1, 2, 2, 2]):
            p = f"layer{i + 1}.0."
            o = F.relu(bn(conv(a, ps[p + "conv1.weight"]), p + "bn1"))
            o = F.relu(bn(conv(o, ps[p + "conv2.weight"], stride, 1, 4), p + "bn2"))
            o = bn(conv(o, ps[p + "conv3.weight"]), p + "bn3")
            a = F.relu(o + bn(conv(a, ps[p + "downsample.0.weight"], stride), p + "downsample.1"))
        logits = F.linear(a.mean((2, 3)), ps["fc.weight"], ps["fc.bias"])
        F.cross_entropy(logits, y).backward()
        return logits.detach(), {k: float(v.grad.double().norm()) for k, v in ps.items()}

    ref_logits, n64 = torch_step(torch.float64)
    _, n32 = torch_step(torch.float32)
    names = list(n64)
    fx = dict(grad_norms_f64=torch.tensor([n64[k] for k in names], dtype=torch.float64), grad_norms=torch.tensor([n32[k] for k in names], dtype=torch.float64))
    emu_env.activate()
    try:
        dev = torch.device("cpu")
        net.materialize(dev).train()
        logits = net(x)
        CrossEntropyLoss()(logits, y).backward()
        assert rel_err(logits.detach().double(), ref_logits.detach()) <= 1e-4
        params = dict(net.named_parameters())
        _grad_check(torch.tensor([float(params[k].grad.double().norm()) for k in names], dtype=torch.float64), fx, "small resnext")
        net.eval()
        with torch.no_grad():
            _folded_eval(net, x, net(x).cpu())
    finally:
        emu_env.deactivate()
