"""ShuffleNetV2 classifiers: the channel-shuffle block with its merge sweeps, the shufflenet_v2 models, the variants the 16-byte contract
refuses, synchronised BatchNorm and a Trainer step.

  reference (its own classification_models/shufflenetv2.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/shufflenet_*.pt elsewhere (tests/make_shufflenet_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars.  A block: tests/test_blocks.py's `_check` - forward output, the running statistics of every BatchNorm in the block and eval output at
2e-5, input and parameter gradients at 1e-4 (relative, max-norm), the folded eval form against the unfolded one at 2e-5.  A whole model:
logits and loss at 1e-4; parameter gradients by tests/test_resnet.py's `_grad_check` (per-parameter norms against the fp64 run of the same
modules, no further from it than 3 x the reference's own fp32 run).

The 1e-4 bar on the training logits is a condition on the input: the fixture writer refuses to write when the reference's own fp32 logits lie
more than a third of the bar from its fp64 logits.  On this input (4 x 3 x 64 x 64, seed 5, deterministic_fill(seed=4)) the reference's own
fp32 run is, against its fp64 run (as the writer printed them when the committed fixtures were made): shufflenet_v2_x0_5 logits 1.1e-5,
gradient norms worst / mean 7.4e-3 / 1.3e-3 (they sit at ReLU flips on its 2 x 2 maps, and move with the CPU's summation order); the custom
model (structure [2, 3, 2], stage widths [8, 16, 32, 64, 128]) 1.3e-6 and 9.1e-6 / 1.3e-6.  shufflenet_v2_x1_5 meets the logits condition
too but its gradient norms sit at such flips as well: it gets a layout-only fixture (keys and shapes, no forward).
"""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc
from test_mobilenet import _check_grads, _grad_check, _model_inputs, _record_step, _wrap

HERE = os.path.dirname(os.path.abspath(__file__))
CUSTOM = dict(structure=[2, 3, 2], stages_out_channels=[8, 16, 32, 64, 128])
MODELS = ["shufflenet_v2_x0_5", "shufflenet_v2_custom5"]
CLS = {"shufflenet_v2_x0_5": "ShufflenetV2_x0_5", "shufflenet_v2_custom5": "CustomizedShuffleNetV2", "shufflenet_v2_x1_5": "ShufflenetV2_x1_5"}
# name: (constructor arguments of every block of the chain, input shape)
BLOCKS = {"stride1": ([(8, 8, 1)], (2, 8, 6, 6)), "stride2": ([(8, 16, 2)], (2, 8, 6, 6)), "stride2_odd": ([(8, 16, 2)], (2, 8, 7, 5)),
          "chain": ([(8, 8, 1), (8, 8, 1)], (2, 8, 6, 6))}


def _arch(name, **extra):
    return dict(CUSTOM, **extra) if name == "shufflenet_v2_custom5" else dict(extra)


# --------------------------------------------------------------------------------------------- reference side (recorded tensors)
def _block_input(shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(1)) + 0.5


def _block_reference():
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.shufflenetv2 as r

        out = {}
        for i, (name, (args, shape)) in enumerate(BLOCKS.items()):
            torch.manual_seed(7 + i)
            blk = nn.Sequential(*[r.ChannelShuffleInvertedResidual(*a) for a in args])
            G.deterministic_fill(blk, seed=11 + i)
            out[name] = _record_step(blk, _block_input(shape), 5 + i)
        return out

    return G.reference_outputs("shufflenet_block_reference", compute)


def _ref_model(r, name, num_classes=10):
    from super_gradients.training.utils.utils import HpmStruct

    return getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=num_classes, **_arch(name)), num_classes=num_classes)


def _model_reference(name):
    def compute():
        import copy

        ref_shim.install()
        import super_gradients.training.models.classification_models.shufflenetv2 as r

        ref = _ref_model(r, name)
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

    return G.reference_outputs(f"shufflenet_{name}_reference", compute)


def _layout_reference():
    """State-dict names and shapes of the variant that gets no forward pass here."""
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.shufflenetv2 as r

        return {"shufflenet_v2_x1_5": [(k, tuple(v.shape)) for k, v in _ref_model(r, "shufflenet_v2_x1_5").state_dict().items()]}

    return G.reference_outputs("shufflenet_layout_reference", compute)


# --------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("cfg", list(BLOCKS))
def test_shuffle_blocks_against_reference(backend, cfg):
    """Training forward, input gradient, every parameter gradient, the running statistics of every BatchNorm after the step, eval forward and
    the folded eval form against the unfolded one.  `chain`: two stride-1 blocks - the second one's chunk is two slice views of the
    interleaved buffer the first one's merge sweep wrote, and both halves of its dx reach the first one's backward."""
    from super_gradients_amd.training.models.classification_models.shufflenetv2 import ChannelShuffleInvertedResidual

    args, shape = BLOCKS[cfg]
    fx = _block_reference()[cfg]
    blocks = [ChannelShuffleInvertedResidual(*a) for a in args]
    net = _wrap(blocks, backend)
    assert list(net.state_dict().keys()) == list(fx["state"].keys())
    assert [tuple(v.shape) for v in net.state_dict().values()] == [tuple(v.shape) for v in fx["state"].values()]
    assert all((b.branch1 is None) == (a[2] == 1) for a, b in zip(args, blocks))
    net.load_state_dict(fx["state"], strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(shape)

    def run(inp):
        for b in blocks:
            inp = b.fwd(inp)
        return inp

    y = run(to_nhwc(x, backend))
    assert_close(to_nchw_cpu(y), fx["y"], 2e-5, "training forward")
    dy = to_nhwc(fx["dy"], backend)
    dy0 = dy.clone()
    d = dy
    for b in reversed(blocks):
        d = b.bwd(d)
    net.join_side()
    assert torch.equal(dy.cpu(), dy0.cpu()), "bwd changed the caller's dy"
    assert_close(to_nchw_cpu(d), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(net, fx, 1e-4)
    n_bn = 0
    for k, b in net.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 2e-5, k)
            n_bn += 1
    assert n_bn == sum(6 if a[2] == 1 else 10 for a in args)
    net.eval()
    with torch.no_grad():
        ye = to_nchw_cpu(run(to_nhwc(x, backend)))
        assert_close(ye, fx["y_eval"], 2e-5, "eval forward")
        net.prep_model_for_conversion()
        assert all(v._folded is not None for b in blocks for v in (b.pw, b.dw, b.pwl))
        assert_close(to_nchw_cpu(run(to_nhwc(x, backend))), ye, 2e-5, "folded against unfolded eval forward")


def test_block_protocol_accumulate_and_addend(backend):
    """SgxBlock.bwd's dx_out / accumulate / addend for both strides: dx_out (+)= dx + addend."""
    from super_gradients_amd.training.models.classification_models.shufflenetv2 import ChannelShuffleInvertedResidual

    for args in ((8, 8, 1), (8, 16, 2)):
        blk = ChannelShuffleInvertedResidual(*args)
        net = _wrap([blk], backend)
        G.deterministic_fill(net, seed=3)
        net.train()
        x = to_nhwc(_block_input((2, 8, 6, 6)), backend)
        g = torch.Generator().manual_seed(9)
        outs = []
        for mode in ("plain", "protocol"):
            net.zero_grad()
            y = blk.fwd(x)
            dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(backend)
            if mode == "plain":
                outs.append(blk.bwd(dy).cpu().clone())
            else:
                prior, addend = torch.randn(x.shape, generator=g).to(backend), torch.randn(x.shape, generator=g).to(backend)
                buf = prior.clone()
                assert blk.bwd(dy, dx_out=buf, accumulate=True, addend=addend) is buf
                outs.append((buf - prior - addend).cpu())
            net.join_side()
        assert_close(outs[1], outs[0], 2e-5, f"dx through dx_out / accumulate / addend {args}")


# --------------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("name", MODELS)
def test_state_dict_layout_matches_reference(name):
    from super_gradients_amd.training import models

    fx = _model_reference(name)
    net = models.get(name, arch_params=_arch(name), num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in fx["state_layout"]]


def test_x1_5_constructs_with_the_reference_layout():
    from super_gradients_amd.training import models

    net = models.get("shufflenet_v2_x1_5", num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in _layout_reference()["shufflenet_v2_x1_5"]]


@pytest.mark.parametrize("name", MODELS)
def test_checkpoint_round_trip_with_reference(name):
    """Both directions, strictly: against the reference's own model class where its tree exists, against a plain state dict of the recorded
    layout elsewhere."""
    from super_gradients_amd.training import models

    net = models.get(name, arch_params=_arch(name), num_classes=10)
    if ref_shim.available():
        ref_shim.install()
        import super_gradients.training.models.classification_models.shufflenetv2 as r

        ref = _ref_model(r, name)
        G.deterministic_fill(ref, seed=9)
        src = ref.state_dict()
        back = _ref_model(r, name)
    else:
        g = torch.Generator().manual_seed(9)
        src = {k: (torch.zeros(s, dtype=torch.long) if k.endswith("num_batches_tracked") else torch.rand(s, generator=g) + 0.5)
               for k, s in _model_reference(name)["state_layout"]}
        back = None
    net.load_state_dict(src, strict=True)
    out = net.state_dict()
    assert list(out) == list(src)
    for k, a in src.items():
        assert torch.equal(a, out[k].cpu()), k
    if back is not None:
        back.load_state_dict(out, strict=True)
        for (k, a), b in zip(src.items(), back.state_dict().values()):
            assert torch.equal(a, b), k


def test_checkpoint_round_trip_between_products(backend):
    """state_dict of a materialised model -> a fresh model -> the same logits (eval), strictly."""
    from super_gradients_amd.training import models

    name = "shufflenet_v2_custom5"
    a = models.get(name, arch_params=_arch(name), num_classes=10)
    G.deterministic_fill(a, seed=9)
    a.materialize(backend).eval()
    sd = {k: v.cpu().clone() for k, v in a.state_dict().items()}
    b = models.get(name, arch_params=_arch(name), num_classes=10)
    b.load_state_dict(sd, strict=True)
    b.materialize(backend).eval()
    x = _model_inputs()[0].to(backend)
    with torch.no_grad():
        assert torch.equal(a(x).cpu(), b(x).cpu())
    for (k, v), w in zip(sd.items(), b.state_dict().values()):
        assert torch.equal(v, w.cpu()), k


def test_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import LinearLayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models.shufflenetv2 import ChannelShuffleInvertedResidual, ShuffleNetV2Base

    net = models.get("shufflenet_v2_x0_5", num_classes=10)
    blocks = [m for m in net.modules() if isinstance(m, ChannelShuffleInvertedResidual)]
    assert [b.stride for b in blocks] == [2, 1, 1, 1] + [2] + [1] * 7 + [2, 1, 1, 1] and [b.h for b in blocks] == [24] * 4 + [48] * 8 + [96] * 4
    assert net.fc.in_features == 1024 and net.fc.out_features == 10
    assert net.get_input_channels() == 3 and not net.supports_half_inference()
    assert net.gradient_buckets() == ["conv1.", "layer2.", "layer3.", "layer4.", "conv5.", "fc."]
    with pytest.raises(NotImplementedError):
        net.half_inference()
    # arch_params.num_classes when num_classes is not given (the reference's `num_classes or arch_params.num_classes`)
    assert models.get("shufflenet_v2_x0_5", arch_params=dict(num_classes=7), num_classes=None).fc.out_features == 7
    net.replace_head(new_num_classes=5)
    assert isinstance(net.fc, LinearLayer) and net.fc.out_features == 5 and list(net.state_dict())[-2:] == ["fc.weight", "fc.bias"]
    assert net.get_finetune_lr_dict(0.1) == {"fc": 0.1, "default": 0.0}
    with pytest.raises(NotImplementedError, match="new_head"):
        net.replace_head(new_head=nn.Linear(1024, 2))
    with pytest.raises(ValueError):
        net.replace_head()
    # the 16-byte contract: the half widths 58 and 122 of stage 2
    for name, width in (("shufflenet_v2_x1_0", "58"), ("shufflenet_v2_x2_0", "122")):
        with pytest.raises(NotImplementedError, match=f"multiple of 4.*{width}"):
            models.get(name, num_classes=10)
    with pytest.raises(NotImplementedError, match="backbone_mode"):
        ShuffleNetV2Base([2, 2, 2], [8, 16, 32, 64, 128], backbone_mode=True)
    with pytest.raises(NotImplementedError, match="stride"):
        ChannelShuffleInvertedResidual(8, 16, 3)
    with pytest.raises(ValueError):
        ShuffleNetV2Base([2, 2], [8, 16, 32, 64, 128])
    custom = models.get("shufflenet_v2_custom5", arch_params=_arch("shufflenet_v2_custom5"), num_classes=3)
    assert custom.structure == [2, 3, 2] and custom.out_channels == [8, 16, 32, 64, 128] and custom.fc.out_features == 3


def _product_against_reference(name, device):
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    fx = _model_reference(name)
    net = models.get(name, arch_params=_arch(name), num_classes=10)
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
def test_product_shufflenet_emulation(name):
    """The whole model on the host emulation of the kernels (CPU tensors): logits, loss, gradient norms, running statistics, eval, folded eval."""
    import emu_env

    emu_env.activate()
    try:
        _product_against_reference(name, torch.device("cpu"))
    finally:
        emu_env.deactivate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_shufflenet_golden(gpu_device, name):
    _product_against_reference(name, gpu_device)


# --------------------------------------------------------------------------------------------- trainer
@pytest.mark.gpu
def test_trainer_step_shufflenet_v2_x0_5(gpu_device, tmp_path):
    """One Trainer step (SGD, cross-entropy) of models.get("shufflenet_v2_x0_5", num_classes=10) at 8 x 3 x 64 x 64: finite loss, every weight
    moves, every BatchNorm counted one batch."""
    from super_gradients_amd.training import Trainer, models
    from test_mobilenet import _train_params

    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(8, 3, 64, 64, generator=g), torch.arange(8) % 10
    loader = [(x, labels)]
    torch.manual_seed(11)
    net = models.get("shufflenet_v2_x0_5", num_classes=10)
    before = {k: v.clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    res = Trainer("s", ckpt_root_dir=str(tmp_path)).train(net, _train_params(1), loader, valid_loader=loader)
    loss = res[-1]["train"]["CrossEntropyLoss"]
    assert loss == loss and abs(loss) < 1e4, res
    sd = net.state_dict()
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    moved = [k for k, v in before.items() if k.endswith("weight") and not torch.equal(v, sd[k].cpu())]
    assert len(moved) == sum(k.endswith("weight") for k in before), "parameters that did not change"
    assert all(bool(torch.isfinite(v.cpu()).all()) for v in sd.values() if v.dtype.is_floating_point)


# --------------------------------------------------------------------------------------------- synchronised BatchNorm
def _custom(device, seed=4):
    from super_gradients_amd.training import models

    net = models.get("shufflenet_v2_custom5", arch_params=_arch("shufflenet_v2_custom5"), num_classes=10)
    G.deterministic_fill(net, seed=seed)
    return net.materialize(device)


def _sync_worker(rank, world, port, outdir):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "emu"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import emu_env

    emu_env.activate()
    import torch.distributed as dist

    dist.init_process_group(backend="gloo", init_method="env://", rank=rank, world_size=world)
    net = _custom(torch.device("cpu")).set_sync_bn(True).train()
    x = _model_inputs()[0]
    half = x.shape[0] // world
    with torch.no_grad():
        logits = net(x[rank * half:(rank + 1) * half])
    torch.save(dict(logits=logits, buffers={k: v.clone() for k, v in net.state_dict().items() if "running_" in k}), os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_sync_bn_two_ranks_match_one_process_with_the_whole_batch(tmp_path):
    """gloo, world size 2, host emulation: two ranks with half the batch each against one process with the whole batch, on the custom model's
    logits and running statistics at 2e-5."""
    world = 2
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_sync_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt")) for i in range(world)]
    import emu_env

    emu_env.activate()
    try:
        net = _custom(torch.device("cpu")).train()
        x = _model_inputs()[0]
        with torch.no_grad():
            whole = net(x)
            local = _custom(torch.device("cpu")).train()(x[:2])
        buffers = {k: v.clone() for k, v in net.state_dict().items() if "running_" in k}
    finally:
        emu_env.deactivate()
    assert_close(torch.cat([r[0]["logits"], r[1]["logits"]]), whole, 2e-5, "logits of the two ranks against the whole batch")
    assert rel_err(r[0]["logits"], local) > 1e-3, "the half batch alone gives the same logits: the check would not see local statistics"
    for k, v in buffers.items():
        for i in range(world):
            assert_close(r[i]["buffers"][k], v, 2e-5, f"rank {i} {k}")
