"""RepVGG classifiers: the three-branch RepVGGBlock (identity BatchNorm), the repvgg_* models and a few Trainer steps.

  reference (its own modules/repvgg_block.py / classification_models/repvgg.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/repvgg_*.pt elsewhere (tests/make_repvgg_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars: 1e-4 relative (max-norm) on activations / logits / loss as tests/test_resnet.py and tests/test_blocks.py; parameter gradients of a
block by tests/test_blocks.py's scheme, of a whole model by tests/test_resnet.py's `_grad_check` (norms against the fp64 run of the same
modules, no further from it than 3 x the reference's own fp32 run: ReLU flips between two fp32 implementations make an element-wise
whole-model comparison meaningless).
"""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc

C_BLOCK = 16
MODELS = ["repvgg_a0", "repvgg_b0"]
CLS = {"repvgg_a0": "RepVggA0", "repvgg_b0": "RepVggB0"}


# --------------------------------------------------------------------------------------------- reference side (recorded tensors)
def _block_input():
    return torch.randn(2, C_BLOCK, 6, 6, generator=torch.Generator().manual_seed(1)) + 0.5


def _stack_input():
    return torch.randn(2, 8, 12, 12, generator=torch.Generator().manual_seed(2)) + 0.5


def _record_step(mod, x, seed):
    """One training step (sum-free: a seeded upstream gradient) and the eval forward after it, of a reference module."""
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
        from super_gradients.modules.repvgg_block import RepVGGBlock as RefBlock

        out = {}
        for ua in (False, True):
            torch.manual_seed(7)
            blk = RefBlock(C_BLOCK, C_BLOCK, use_alpha=ua)
            G.deterministic_fill(blk, seed=11)
            out[f"alpha{int(ua)}"] = _record_step(blk, _block_input(), 5)
        torch.manual_seed(8)
        stack = nn.Sequential(RefBlock(8, C_BLOCK, stride=2), RefBlock(C_BLOCK, C_BLOCK), RefBlock(C_BLOCK, C_BLOCK))
        G.deterministic_fill(stack, seed=12)
        out["stack"] = _record_step(stack, _stack_input(), 6)
        return out

    return G.reference_outputs("repvgg_block_identity_reference", compute)


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)


def _sample_index(numel, i):
    return torch.randint(0, numel, (min(numel, 32),), generator=torch.Generator().manual_seed(1000 + i))


def _model_reference(name):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.repvgg as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10, build_residual_branches=True))
        G.deterministic_fill(ref, seed=4)
        layout = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        x, y = _model_inputs()
        ref64 = copy.deepcopy(ref).double()
        nn.Module.train(ref, True)  # (the reference's own train() returns None)
        nn.Module.train(ref64, True)
        logits = ref(x)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        logits64 = ref64(x.double())
        F.cross_entropy(logits64, y).backward()
        names = [k for k, _ in ref.named_parameters()]
        p32, p64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
        sample = torch.cat([p32[k].grad.flatten()[_sample_index(p32[k].numel(), i)] for i, k in enumerate(names)])
        sample64 = torch.cat([p64[k].grad.flatten()[_sample_index(p64[k].numel(), i)] for i, k in enumerate(names)])
        checks = {k: float(v.double().sum()) for k, v in ref.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")}
        nn.Module.train(ref, False)
        with torch.no_grad():
            eval_logits = ref(x)
            r.fuse_repvgg_blocks_residual_branches(ref)
            fused_logits = ref(x)
        return dict(state_layout=layout, logits=logits.detach(), loss=loss.detach(), logits_f64=logits64.detach(), grad_names=names,
                    grad_norms=torch.tensor([float(p32[k].grad.double().norm()) for k in names], dtype=torch.float64),
                    grad_norms_f64=torch.tensor([float(p64[k].grad.norm()) for k in names], dtype=torch.float64), grad_sample=sample,
                    grad_sample_f64=sample64, bn_running_checksum=checks, eval_logits=eval_logits, fused_logits=fused_logits,
                    fused_keys=list(ref.state_dict().keys()))

    return G.reference_outputs(f"{name}_reference", compute)


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
        if "rbr_reparam" in name:
            continue
        rg = fx["grads"][name]
        e = float((p.grad.cpu().double().reshape(rg.shape) - rg.double()).abs().max()) / max(float(rg.abs().max()), 1e-2 * gmax)
        assert e <= tol, f"grad {name}: {e:.3e}"


@pytest.mark.parametrize("use_alpha", [False, True])
def test_identity_block_against_reference(backend, use_alpha):
    """RepVGGBlock with the identity-BatchNorm branch against the reference's block: training forward, input gradient, every parameter
    gradient (alpha's included), running statistics after the step, eval forward, and the fused form against the unfused one."""
    from super_gradients_amd.modules.repvgg_block import RepVGGBlock

    fx = _block_reference()[f"alpha{int(use_alpha)}"]
    blk = RepVGGBlock(C_BLOCK, C_BLOCK, use_alpha=use_alpha)
    assert blk.no_conv_branch is not None
    assert list(blk.state_dict().keys()) == list(fx["state"].keys())  # no_conv_branch.* first (after alpha), as in the reference
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k}": v for k, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input()
    y = blk.fwd(to_nhwc(x, backend))
    assert_close(to_nchw_cpu(y), fx["y"], 1e-4, "training forward")
    dx = blk.bwd(to_nhwc(fx["dy"], backend))
    net.join_side()
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(blk, fx, 1e-4)
    for k, b in blk.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 1e-4, k)
    net.eval()
    with torch.no_grad():
        ye = to_nchw_cpu(blk.fwd(to_nhwc(x, backend)))
        assert_close(ye, fx["y_eval"], 1e-4, "eval forward")
        blk.fuse_block_residual_branches()
        assert tuple(blk.rbr_reparam.weight.shape) == (C_BLOCK, C_BLOCK, 3, 3)
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend))), ye, 2e-5, "fused against unfused (fp32 round-off)")
    with pytest.raises(RuntimeError):
        net.train()
        blk.fwd(to_nhwc(x, backend))


def test_stacked_blocks_hand_statistics_on(backend):
    """A stride-2 two-branch block and two identity blocks behind it, as in a RepVGG stage: each forward sweep hands the statistics rows of
    its output to the next block's identity BatchNorm.  Against the reference's stack, and against the same blocks fed by a standalone
    statistics sweep (the rows then come from another kernel: equal within fp32 round-off of the rows, 1e-6 relative)."""
    from super_gradients_amd.modules.repvgg_block import RepVGGBlock

    fx = _block_reference()["stack"]

    def build():
        blocks = [RepVGGBlock(8, C_BLOCK, stride=2), RepVGGBlock(C_BLOCK, C_BLOCK), RepVGGBlock(C_BLOCK, C_BLOCK)]
        net = _wrap(blocks, backend)
        net.load_state_dict(fx["state"], strict=True)
        net.train()
        net.zero_grad()
        return net, blocks

    def run(net, blocks, hand_over):
        a, stats = to_nhwc(_stack_input(), backend), None
        for i, b in enumerate(blocks):
            want = hand_over and i + 1 < len(blocks)
            a = b.fwd(a, x_stats=stats, want_stats=want)
            stats = b.take_stats() if want else None
            assert (stats is not None) == want
        d = to_nhwc(fx["dy"], backend)
        for b in reversed(blocks):
            d = b.bwd(d)
        net.join_side()
        return to_nchw_cpu(a), to_nchw_cpu(d)

    assert [k for k, _ in build()[0].state_dict().items()] == list(fx["state"].keys())
    net, blocks = build()
    y, dx = run(net, blocks, True)
    assert_close(y, fx["y"], 1e-4, "forward of the stack")
    assert_close(dx, fx["x_grad"], 1e-4, "input gradient of the stack")
    _check_grads(net, fx, 1e-4)
    for k, b in net.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 1e-4, k)
    net2, blocks2 = build()
    y2, dx2 = run(net2, blocks2, False)
    assert_close(y, y2, 1e-6, "handed-over rows against a standalone statistics sweep: forward")
    assert_close(dx, dx2, 1e-5, "handed-over rows against a standalone statistics sweep: input gradient")
    for (k, b), b2 in zip(net.named_buffers(), net2.buffers()):
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), b2.cpu(), 1e-6, k)


def test_deployment_form_block_loads_a_fused_checkpoint(backend):
    """build_residual_branches=False: only rbr_reparam.{weight,bias} in the state, inference-only, reproduces the fused block."""
    from super_gradients_amd.modules.repvgg_block import RepVGGBlock, fuse_repvgg_blocks_residual_branches

    fx = _block_reference()["alpha0"]
    blk = RepVGGBlock(C_BLOCK, C_BLOCK)
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k}": v for k, v in fx["state"].items()}, strict=True)
    with pytest.raises(RuntimeError):
        fuse_repvgg_blocks_residual_branches(net)  # training mode
    net.eval()
    fuse_repvgg_blocks_residual_branches(net)
    dep = RepVGGBlock(C_BLOCK, C_BLOCK, build_residual_branches=False)
    assert sorted(dep.state_dict().keys()) == ["rbr_reparam.bias", "rbr_reparam.weight"]
    dnet = _wrap([dep], backend).eval()
    dnet.load_state_dict({"0.rbr_reparam.weight": blk.rbr_reparam.weight.detach().cpu(), "0.rbr_reparam.bias": blk.rbr_reparam.bias.detach().cpu()}, strict=True)
    x = to_nhwc(_block_input(), backend)
    with torch.no_grad():
        assert torch.equal(dep.fwd(x).cpu(), blk.fwd(x).cpu())


# --------------------------------------------------------------------------------------------- models
def test_registered_variants_and_refusals():
    from super_gradients_amd.modules.repvgg_block import RepVGGBlock
    from super_gradients_amd.training import models

    structs = {"repvgg_a0": ([2, 4, 14, 1], 1280), "repvgg_a1": ([2, 4, 14, 1], 1280), "repvgg_a2": ([2, 4, 14, 1], 1408), "repvgg_b0": ([4, 6, 16, 1], 1280),
               "repvgg_b1": ([4, 6, 16, 1], 2048), "repvgg_b2": ([4, 6, 16, 1], 2560), "repvgg_b3": ([4, 6, 16, 1], 2560), "repvgg_d2se": ([8, 14, 24, 1], 2560)}
    for name, (struct, width) in structs.items():
        net = models.get(name, num_classes=7)
        assert [len(getattr(net, f"stage{i + 1}").blocks()) for i in range(4)] == struct, name
        assert net.linear.in_features == width and net.linear.out_features == 7, name
        for i in range(4):
            blocks = getattr(net, f"stage{i + 1}").blocks()
            assert blocks[0].no_conv_branch is None and all(b.no_conv_branch is not None for b in blocks[1:]), name
    net = models.get("repvgg_custom", arch_params=dict(struct=[1, 2, 1, 1], width_multiplier=[0.25, 0.25, 0.25, 0.5]), num_classes=3)
    assert sum(isinstance(m, RepVGGBlock) for m in net.modules()) == 6 and net.train() is net
    net.replace_head(new_num_classes=5)
    assert net.linear.out_features == 5 and net.get_finetune_lr_dict(0.1) == {"linear": 0.1, "default": 0}
    for bad in (dict(use_se=True), dict(backbone_mode=True), dict(width_multiplier=[0.1, 0.25, 0.25, 0.5])):
        with pytest.raises(NotImplementedError):
            models.get("repvgg_custom", arch_params=dict(dict(struct=[1, 1, 1, 1], width_multiplier=[0.25] * 4), **bad), num_classes=3)
    dep = models.get("repvgg_a0", arch_params=dict(build_residual_branches=False), num_classes=10)
    assert not dep.training and all(k.split(".")[-2] in ("rbr_reparam", "linear") for k in dep.state_dict())
    with pytest.raises(AssertionError):
        dep.train()


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
    import super_gradients.training.models.classification_models.repvgg as r
    from super_gradients.training.utils.utils import HpmStruct

    ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10, build_residual_branches=True))
    G.deterministic_fill(ref, seed=9)
    net = models.get(name, num_classes=10)
    net.load_state_dict(ref.state_dict(), strict=True)
    back = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10, build_residual_branches=True))
    back.load_state_dict(net.state_dict(), strict=True)
    for (k, a), b in zip(ref.state_dict().items(), back.state_dict().values()):
        assert torch.equal(a, b), k


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
    assert e_pair <= 1e-4 or e_hip <= max(1e-4, 2.0 * e_cpu), f"logits: hip-ref32 {e_pair:.2e} hip-ref64 {e_hip:.2e} ref32-ref64 {e_cpu:.2e}"
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-4 * abs(float(fx["loss"]))
    params = dict(net.named_parameters())
    _grad_check(torch.tensor([float(params[n].grad.double().norm()) for n in fx["grad_names"]], dtype=torch.float64), fx, name)
    # the seeded sample of gradient elements, as one vector: relative L2 against fp64 no worse than 3 x the reference's own fp32 run
    sample = torch.cat([params[k].grad.cpu().flatten()[_sample_index(params[k].numel(), i)] for i, k in enumerate(fx["grad_names"])]).double()
    s64 = fx["grad_sample_f64"]
    l2_h, l2_c = float((sample - s64).norm() / s64.norm()), float((fx["grad_sample"].double() - s64).norm() / s64.norm())
    print(f"{name}: sampled gradient elements, relative L2 vs fp64: hip {l2_h:.2e}, reference fp32 {l2_c:.2e}")
    assert l2_h <= max(1e-3, 3.0 * l2_c), f"sampled gradient elements vs fp64: hip {l2_h:.2e}, reference fp32 {l2_c:.2e}"
    for k, v in fx["bn_running_checksum"].items():
        assert abs(float(net.state_dict()[k].double().sum()) - v) <= 1e-4 * max(abs(v), 1.0), k
    # eval, re-parameterisation, deployment form
    net.eval()
    with torch.no_grad():
        ev = net(x.to(device)).cpu()
        assert rel_err(ev, fx["eval_logits"]) <= 1e-4, f"eval logits {rel_err(ev, fx['eval_logits']):.2e}"
        with pytest.raises(RuntimeError):
            nn.Module.train(net, True)
            net.prep_model_for_conversion()
        net.eval()
        net.prep_model_for_conversion()
        fused = net(x.to(device)).cpu()
    print(f"{name}: fused against unfused eval logits {rel_err(fused, ev):.2e}")
    assert rel_err(fused, ev) <= 2e-5, f"prep_model_for_conversion changed the eval logits by {rel_err(fused, ev):.2e}"
    assert list(net.state_dict().keys()) == fx["fused_keys"]
    dep = models.get(name, arch_params=dict(build_residual_branches=False), num_classes=10)
    assert list(dep.state_dict().keys()) == fx["fused_keys"]
    dep.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()}, strict=True)
    dep.materialize(device)
    with torch.no_grad():
        assert torch.equal(dep(x.to(device)).cpu(), fused), "the deployment-form model does not reproduce the fused model's logits"


@pytest.mark.parametrize("name", MODELS)
def test_product_repvgg_emulation(name):
    """The whole model on the host emulation of the kernels (CPU tensors): logits, loss, gradients, running statistics, fusion, deployment form."""
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference(name, torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_repvgg_golden(gpu_device, name):
    _product_against_reference(name, gpu_device)


# --------------------------------------------------------------------------------------------- trainer
def _train_params(epochs, **kw):
    """recipes/training_hyperparams/imagenet_repvgg_train_params.yaml as a plain dict (max_epochs shortened; lr 0.1 as the recipe)."""
    return dict(max_epochs=epochs, lr_mode="CosineLRScheduler", initial_lr=0.1, cosine_final_lr_ratio=0, loss="CrossEntropyLoss", optimizer="SGD",
                optimizer_params=dict(momentum=0.9, weight_decay=1e-4), zero_weight_decay_on_bias_and_bn=True, average_best_models=True,
                metric_to_watch="Accuracy", greater_metric_to_watch_is_better=True, train_metrics_list=["Accuracy", "Top5"],
                valid_metrics_list=["Accuracy", "Top5"], silent_mode=True, seed=3, **kw)


def test_trainer_steps_with_the_imagenet_repvgg_recipe(backend, tmp_path):
    """A few epochs of Trainer.train() on a small RepVGG (repvgg_custom) and a synthetic, learnable loader: the loss falls, the checkpoint
    resumes to the same weights, and set_sync_bn(True) reaches the identity BatchNorm."""
    from super_gradients_amd.modules.layers import BatchNorm
    from super_gradients_amd.training import Trainer, models
    from super_gradients_amd.training.utils.callbacks import Callback

    arch = dict(struct=[2, 2, 1, 1], width_multiplier=[0.125, 0.125, 0.0625, 0.03125])
    g = torch.Generator().manual_seed(2)
    bs, size = (8, 32) if backend.type == "cuda" else (4, 16)
    labels = torch.arange(bs) % 6
    # class k lights up channel k % 3 in one half of the image: learnable in a few steps
    x = torch.randn(bs, 3, size, size, generator=g) * 0.3
    for i, k in enumerate(labels.tolist()):
        x[i, k % 3, :, (k // 3) * (size // 2):(k // 3 + 1) * (size // 2)] += 2.0
    loader = [(x, labels)] * 3

    def make():
        torch.manual_seed(11)
        net = models.get("repvgg_custom", arch_params=dict(arch), num_classes=6)
        if backend.type != "cuda":
            net.materialize(backend)
        return net

    net = make()
    assert net.set_sync_bn(True) is net and all(m.sync for m in net.modules() if isinstance(m, BatchNorm))
    assert sum(1 for n, m in net.named_modules() if n.endswith("no_conv_branch") and isinstance(m, BatchNorm) and m.sync) == 2
    res = Trainer("a", ckpt_root_dir=str(tmp_path)).train(net, _train_params(4), loader, valid_loader=loader[:1])
    losses = [r["train"]["CrossEntropyLoss"] for r in res]
    assert losses[-1] < 0.7 * losses[0], losses
    assert {"Accuracy", "Top5"} <= set(res[-1]["valid"]) and {"Accuracy", "Top5"} <= set(res[-1]["train"])

    class StopAfterFirst(Callback):
        def on_train_loader_end(self, context):
            context.stop_training = True

    net_b = make()
    Trainer("b", ckpt_root_dir=str(tmp_path)).train(net_b, _train_params(4, phase_callbacks=[StopAfterFirst()]), loader, valid_loader=loader[:1])
    net_c = make()
    Trainer("c", ckpt_root_dir=str(tmp_path)).train(net_c, _train_params(4, resume_path=os.path.join(str(tmp_path), "b", "ckpt_latest.pth")), loader,
                                                    valid_loader=loader[:1])
    for (k, va), vc in zip(net.state_dict().items(), net_c.state_dict().values()):
        if va.dtype.is_floating_point:
            assert torch.allclose(va.cpu(), vc.cpu(), rtol=1e-5, atol=1e-6), k  # (tests/test_api.py::test_trainer_resume's bar)
