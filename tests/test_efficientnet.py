"""EfficientNet classifiers: the MBConv block (expansion, depthwise 3x3 / 5x5 at stride 1 / 2, squeeze-excitation AFTER the SiLU with padded
hidden widths, identity skip, drop-connect), the static "same" padding rule, the efficientnet_* models and Trainer steps.

  reference (its own classification_models/efficientnet.py through the import shim)  ->  recorded tensors   CPU
      live where the reference tree exists, tests/golden/efficientnet_*.pt elsewhere (tests/make_efficientnet_golden.py writes them)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bars as tests/test_mobilenetv3.py.  A block: forward output, running statistics and eval output at 2e-5, input and parameter gradients at
1e-4 (relative, max-norm).  A whole model (drop_connect_rate = 0, dropout_rate = 0 on both sides): logits and loss at 1e-4, parameter
gradients by tests/test_resnet.py's `_grad_check`.  On this input (4 x 3 x 64 x 64, seed 5) the reference's own fp32 run is, against its fp64
run (tests/make_efficientnet_golden.py prints it): logits 4.0e-6 (efficientnet_b0) / 9.7e-6 (efficientnet_b2), per-parameter gradient norms
overall 9.7e-7 / 2.0e-6 - inside a third of the 1e-4 bar.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_util as G
from oracle import ref_shim
from test_mobilenetv3 import _check_grads, _grad_check, _record_step, _wrap
from util import assert_close, rel_err, to_nchw_cpu, to_nhwc

MODELS = ["efficientnet_b0", "efficientnet_b2"]
CLS = {"efficientnet_b0": "EfficientNetB0", "efficientnet_b1": "EfficientNetB1", "efficientnet_b2": "EfficientNetB2", "efficientnet_b3": "EfficientNetB3",
       "efficientnet_b4": "EfficientNetB4", "efficientnet_b5": "EfficientNetB5", "efficientnet_b6": "EfficientNetB6", "efficientnet_b7": "EfficientNetB7",
       "efficientnet_b8": "EfficientNetB8", "efficientnet_l2": "EfficientNetL2"}
VARIANTS = {"efficientnet_b0": (1.0, 1.0, 224, 0.2), "efficientnet_b1": (1.0, 1.1, 240, 0.2), "efficientnet_b2": (1.1, 1.2, 260, 0.3),
            "efficientnet_b3": (1.2, 1.4, 300, 0.3), "efficientnet_b4": (1.4, 1.8, 380, 0.4), "efficientnet_b5": (1.6, 2.2, 456, 0.4),
            "efficientnet_b6": (1.8, 2.6, 528, 0.5), "efficientnet_b7": (2.0, 3.1, 600, 0.5), "efficientnet_b8": (2.2, 3.6, 672, 0.5),
            "efficientnet_l2": (4.3, 5.3, 800, 0.5)}
# (block string, stride as the block receives it - EfficientNet's repeats get the int 1, and only then the reference's `stride == 1` skip test
# passes -, configured image_size): expand 1, k3, no skip; expand 6, k3, stride 2 on an even size (hidden 96, SE hidden 4); expand 6, k5,
# stride 1 with skip (SE hidden 10: the padded case); k5, stride 2; k3, stride 2 configured for an odd size
BLOCKS = {
    "e1k3": ("r1_k3_s11_e1_i32_o16_se0.25", [1], 6),
    "e6k3s2": ("r1_k3_s22_e6_i16_o24_se0.25", [2], 6),
    "e6k5skip": ("r1_k5_s11_e6_i40_o40_se0.25", 1, 6),
    "e6k5s2": ("r1_k5_s22_e6_i24_o40_se0.25", [2], 6),
    "e6k3s2odd": ("r1_k3_s22_e6_i16_o24_se0.25", [2], 7),
}
PADS = {"e1k3": (1, 1, 1, 1), "e6k3s2": (1, 0, 1, 0), "e6k5skip": (2, 2, 2, 2), "e6k5s2": (2, 1, 2, 1), "e6k3s2odd": (1, 1, 1, 1)}
BN_MOM, BN_EPS = 0.99, 1e-3
DC_SEED, DC_RATE, DC_BATCH = 2, 0.5, 4  # (seed 2: images 0 and 2 kept, 1 and 3 dropped)


def _block_args(decoder, cfg):
    string, stride, _ = BLOCKS[cfg]
    return decoder.decode([string])[0]._replace(stride=stride)


def _block_input(c, batch=2):
    return torch.randn(batch, c, 6, 6, generator=torch.Generator().manual_seed(1)) + 0.5


def _block_reference():
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.efficientnet as r

        out = {}
        for i, cfg in enumerate(BLOCKS):
            torch.manual_seed(7 + i)
            args = _block_args(r.BlockDecoder, cfg)
            blk = r.MBConvBlock(args, BN_MOM, BN_EPS, image_size=BLOCKS[cfg][2])
            G.deterministic_fill(blk, seed=11 + i)
            out[cfg] = _record_step(blk, _block_input(args.input_filters), 5 + i)
            pad = blk._depthwise_conv.static_padding
            out[cfg]["pad"] = tuple(pad.padding) if hasattr(pad, "padding") else (0, 0, 0, 0)
        return out

    return G.reference_outputs("efficientnet_block_reference", compute)


def _drop_connect_reference():
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.efficientnet as r

        # drop-connect on the skip block: the reference draws torch.rand([B, 1, 1, 1]) exactly once per block forward
        args = _block_args(r.BlockDecoder, "e6k5skip")
        blk = r.MBConvBlock(args, BN_MOM, BN_EPS, image_size=6)
        G.deterministic_fill(blk, seed=31)
        torch.manual_seed(DC_SEED)
        keep = torch.floor(1 - DC_RATE + torch.rand([DC_BATCH, 1, 1, 1])).view(DC_BATCH)
        assert 0 < float(keep.sum()) < DC_BATCH, "the drop-connect seed must keep at least one image and drop at least one"

        class Dc(nn.Module):
            def __init__(self):
                super().__init__()
                self.blk = blk

            def forward(self, x):
                if self.training:
                    torch.manual_seed(DC_SEED)
                return self.blk(x, drop_connect_rate=DC_RATE)

        rec = _record_step(Dc(), _block_input(args.input_filters, DC_BATCH), 17)
        for part in ("state", "grads", "buffers"):
            rec[part] = {k[len("blk."):]: v for k, v in rec[part].items()}
        rec["keep"] = keep
        blk.train()
        torch.manual_seed(DC_SEED)
        blk(_block_input(args.input_filters, DC_BATCH), drop_connect_rate=DC_RATE)
        after_block = torch.get_rng_state()
        torch.manual_seed(DC_SEED)
        torch.rand([DC_BATCH, 1, 1, 1])
        assert torch.equal(after_block, torch.get_rng_state()), "the reference block draws torch.rand([B, 1, 1, 1]) exactly once"
        return rec

    return G.reference_outputs("efficientnet_drop_connect_reference", compute)


def _model_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)


ARCH = dict(drop_connect_rate=0.0, dropout_rate=0.0)
CUSTOM = dict(width_coefficient=0.5, depth_coefficient=0.3, res=32, dropout_rate=0.0, drop_connect_rate=0.0)


def _run_reference(ref, x, y):
    import copy

    layout = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
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


def _model_reference(name):
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.efficientnet as r
        from super_gradients.training.utils.utils import HpmStruct

        ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10, **ARCH))
        G.deterministic_fill(ref, seed=4)
        return _run_reference(ref, *_model_inputs())

    return G.reference_outputs(f"efficientnet_{name}_reference", compute)


def _host_reference():
    """Numbers and layouts the host-only tests compare with: rounding of every variant, block strings, state layouts of B0 / B2 / B7."""
    def compute():
        ref_shim.install()
        import super_gradients.training.models.classification_models.efficientnet as r
        from super_gradients.training.utils.utils import HpmStruct

        out = dict(filters={}, repeats={}, blocks=[tuple(a) for a in r.get_efficientnet_params(1.0, 1.0, 224, 0.2, HpmStruct(num_classes=10))[0]], layouts={})
        for name, (w, d, _, _) in VARIANTS.items():
            out["filters"][name] = [r.round_filters(f, w, 8, None) for f in (16, 24, 32, 40, 80, 112, 192, 320, 1280)]
            out["repeats"][name] = [r.round_repeats(n, d) for n in (1, 2, 3, 4)]
        for name in ("efficientnet_b0", "efficientnet_b2", "efficientnet_b7"):
            ref = getattr(r, CLS[name])(arch_params=HpmStruct(num_classes=10))
            out["layouts"][name] = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        return out

    return G.reference_outputs("efficientnet_host_reference", compute)


# --------------------------------------------------------------------------------------------- blocks
def _product_block(cfg, name="blk"):
    from super_gradients_amd.training.models.classification_models.efficientnet import BlockDecoder, MBConvBlock

    return MBConvBlock(_block_args(BlockDecoder, cfg), BN_MOM, BN_EPS, image_size=BLOCKS[cfg][2], name=name)


@pytest.mark.parametrize("cfg", list(BLOCKS))
def test_mbconv_block_against_reference(backend, cfg):
    """The product block against the reference's MBConvBlock on 2 x C x 6 x 6: state keys and shapes, the reference's pad tuple, training
    forward, input gradient, every parameter gradient (the SE convolutions included), running statistics after the step, eval forward, and
    the folded eval form against the unfolded one."""
    from super_gradients_amd.modules.se_blocks import MBConvSE

    fx = _block_reference()[cfg]
    blk = _product_block(cfg)
    args = blk._block_args
    assert list(blk.state_dict().keys()) == list(fx["state"].keys())
    assert [tuple(v.shape) for v in blk.state_dict().values()] == [tuple(v.shape) for v in fx["state"].values()]
    assert blk.static_padding == tuple(fx["pad"]) == PADS[cfg]
    assert blk._skip == (cfg == "e6k5skip") and isinstance(blk._dw._gate[0], MBConvSE) and blk._dw._gate[0].after_act
    assert blk._se.hidden == max(1, int(args.input_filters * 0.25)) and (blk._se._hp != blk._se.hidden) == (cfg in ("e6k5skip", "e6k5s2"))
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k_}": v for k_, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(args.input_filters)
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
        assert blk._dw._folded is not None and blk._pwl._folded is not None
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend))), ye, 2e-5, "folded against unfolded eval forward")
    net.train()
    assert blk._dw._folded is None


def test_even_configured_layer_refuses_an_odd_input(backend):
    """3x3 stride 2 configured for 6 rows pads (1, 0): on 7 rows the reference yields 3 rows, the kernels' symmetric padding 4 - refused, with
    the layer's name.  The same block configured for an odd size takes both."""
    blk = _product_block("e6k3s2", name="_blocks.3")
    _wrap([blk], backend).eval()
    x = torch.randn(2, 16, 7, 7, generator=torch.Generator().manual_seed(2))
    with pytest.raises(NotImplementedError, match=r"_blocks\.3\._depthwise_conv"):
        blk.fwd(to_nhwc(x, backend))
    odd = _product_block("e6k3s2odd")
    _wrap([odd], backend).eval()
    with torch.no_grad():
        assert tuple(odd.fwd(to_nhwc(x, backend)).shape) == (2, 4, 4, 24)
        assert tuple(odd.fwd(to_nhwc(x[..., :6, :6].contiguous(), backend)).shape) == (2, 3, 3, 24)


def test_drop_connect_against_reference(backend):
    """The skip block at rate 0.5, batch 4, with the reference's keep mask injected: the block bars."""
    fx = _drop_connect_reference()
    torch.manual_seed(DC_SEED)
    keep = torch.floor(1 - DC_RATE + torch.rand([DC_BATCH, 1, 1, 1])).view(DC_BATCH)
    assert torch.equal(keep, fx["keep"]) and 0 < float(keep.sum()) < DC_BATCH
    blk = _product_block("e6k5skip")
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k_}": v for k_, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    x = _block_input(40, DC_BATCH)
    blk._test_keep_mask = keep
    y = to_nchw_cpu(blk.fwd(to_nhwc(x, backend), drop_connect_rate=DC_RATE))
    assert_close(y, fx["y"], 2e-5, "training forward")
    assert torch.equal(y[keep == 0], x[keep == 0]), "a dropped image is the block's input, bit for bit"
    dx = blk.bwd(to_nhwc(fx["dy"], backend))
    net.join_side()
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(blk, fx, 1e-4)
    for k_, b in blk.named_buffers():
        if not k_.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k_], 2e-5, k_)
    net.eval()
    with torch.no_grad():
        assert_close(to_nchw_cpu(blk.fwd(to_nhwc(x, backend), drop_connect_rate=DC_RATE)), fx["y_eval"], 2e-5, "eval forward ignores the rate")


def test_drop_connect_own_mask(backend):
    """With its own Philox mask: two steps after the same torch.manual_seed are equal, another seed differs (a dropped image is the
    block's input itself: that is how the masks are read), eval ignores the rate."""
    blk = _product_block("e6k5skip")
    G.deterministic_fill(blk, seed=31)
    net = _wrap([blk], backend)
    net.train()
    x = _block_input(40, 8)
    dy = torch.randn(8, 40, 6, 6, generator=torch.Generator().manual_seed(4))

    def step(seed):
        torch.manual_seed(seed)
        net.zero_grad()
        y = to_nchw_cpu(blk.fwd(to_nhwc(x, backend), drop_connect_rate=0.5))
        dx = to_nchw_cpu(blk.bwd(to_nhwc(dy, backend)))
        net.join_side()
        return y, dx

    outs = {s: step(s) for s in (1, 2, 3, 4, 5, 6)}
    y1, dx1 = step(1)
    assert torch.equal(y1, outs[1][0]) and torch.equal(dx1, outs[1][1]), "the same seed gives the same step"
    masks = {s: tuple(bool(torch.equal(y[i], x[i])) for i in range(8)) for s, (y, _) in outs.items()}
    assert len(set(masks.values())) > 1, "six seeds gave one mask"
    assert any(any(m) and not all(m) for m in masks.values()), "no seed gave a mixed mask"
    net.eval()
    with torch.no_grad():
        e0 = to_nchw_cpu(blk.fwd(to_nhwc(x, backend), drop_connect_rate=0.0))
        assert torch.equal(to_nchw_cpu(blk.fwd(to_nhwc(x, backend), drop_connect_rate=0.9)), e0), "eval ignores the rate"


# --------------------------------------------------------------------------------------------- host-only
def test_rounding_and_block_strings_match_reference():
    from super_gradients_amd.training.models.classification_models import efficientnet as E

    fx = _host_reference()
    blocks = E.get_efficientnet_params(1.0, 1.0, 224, 0.2, E.HpmStruct(num_classes=10))[0]
    assert [tuple(a) for a in blocks] == [tuple(a) for a in fx["blocks"]]
    a = E.BlockDecoder.decode(["r1_k3_s11_e1_i32_o16_se0.25_noskip"])[0]
    assert a == E.BlockArgs(1, 3, [1], 1, 32, 16, 0.25, False)
    for name, (w, d, res, drop) in VARIANTS.items():
        assert [E.round_filters(f, w, 8, None) for f in (16, 24, 32, 40, 80, 112, 192, 320, 1280)] == fx["filters"][name], name
        assert [E.round_repeats(n, d) for n in (1, 2, 3, 4)] == fx["repeats"][name], name
    assert E.round_filters(32, None, 8, None) == 32 and E.round_repeats(3, None) == 3 and E.round_filters(10, 1.0, 8, 16) == 16


def test_registered_variants_helpers_and_refusals():
    from super_gradients_amd.modules.layers import DepthwiseConvLayer, LinearLayer
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.classification_models import efficientnet as E

    from super_gradients_amd.common.registry import ARCHITECTURES

    assert all(n in ARCHITECTURES for n in list(VARIANTS) + ["CustomizedEfficientnet"])
    for name in ("efficientnet_b0", "efficientnet_b2"):
        w, d, res, drop = VARIANTS[name]
        net = models.get(name, num_classes=7)
        assert isinstance(net, E.EfficientNet) and net._fc.out_features == 7 and net._dropout.p == drop and net.drop_connect_rate == 0.2
        assert net._bn0.momentum == pytest.approx(0.01) and net._bn0.eps == 1e-3 and net._blocks[3]._bn1.momentum == pytest.approx(0.01)
        assert net.get_input_channels() == 3 and not net.supports_half_inference()
        assert net.gradient_buckets() == ["_conv_stem.", "_bn0."] + [f"_blocks.{i}." for i in range(len(net._blocks))] + ["_conv_head.", "_bn1.", "_fc."]
        pads = {b.static_padding for b in net._blocks} | {net._stem_pad.static_padding}
        assert pads <= {(1, 1, 1, 1), (1, 0, 1, 0), (2, 2, 2, 2), (2, 1, 2, 1)}, pads
    b0 = models.get("efficientnet_b0", num_classes=7)
    assert len(b0._blocks) == 16 and sum(b._skip for b in b0._blocks) == 9 and sum(isinstance(m, DepthwiseConvLayer) and m.kernel_size == 5 for m in b0.modules()) == 9
    assert [b._se.hidden for b in b0._blocks][:6] == [8, 4, 6, 6, 10, 10]
    over = models.get("efficientnet_b0", arch_params=dict(drop_connect_rate=0.1, dropout_rate=0.5, batch_norm_momentum=0.9, image_size=96), num_classes=3)
    assert over.drop_connect_rate == 0.1 and over._dropout.p == 0.5 and over._bn1.momentum == pytest.approx(0.1) and over._stem_pad.static_padding == (1, 0, 1, 0)
    custom = models.get("CustomizedEfficientnet", arch_params=dict(CUSTOM), num_classes=3)
    assert len(custom._blocks) == 8 and custom._conv_stem.out_channels == 16
    net = models.get("efficientnet_b0", num_classes=1000)
    net.replace_head(new_num_classes=5)
    assert isinstance(net._fc, LinearLayer) and (net._fc.in_features, net._fc.out_features) == (1280, 5) and list(net.state_dict())[-2:] == ["_fc.weight", "_fc.bias"]
    assert net.get_finetune_lr_dict(0.1) == {"_fc": 0.1, "default": 0.0}
    with pytest.raises(NotImplementedError):
        net.replace_head(new_head=nn.Linear(1280, 2))
    with pytest.raises(ValueError):
        net.replace_head()
    one = models.get("efficientnet_b0", num_classes=4, num_input_channels=1)
    assert one.get_input_channels() == 1 and tuple(one.state_dict()["_conv_stem.weight"].shape) == (32, 1, 3, 3)
    # refusals: dynamic same padding, a 7x7 depthwise filter, widths that are no multiple of 4 (depth_divisor 6 gives a stem of 30)
    with pytest.raises(NotImplementedError, match="image_size"):
        models.get("efficientnet_b0", arch_params=dict(image_size=None), num_classes=3)
    with pytest.raises(NotImplementedError, match="kernel size"):
        E.MBConvBlock(E.BlockDecoder.decode(["r1_k7_s11_e1_i32_o16_se0.25"])[0], BN_MOM, BN_EPS, image_size=8)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        E.MBConvBlock(E.BlockDecoder.decode(["r1_k3_s11_e1_i32_o18_se0.25"])[0], BN_MOM, BN_EPS, image_size=8)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        models.get("efficientnet_b0", arch_params=dict(depth_divisor=6), num_classes=3)
    with pytest.raises(NotImplementedError):
        net.half_inference()


@pytest.mark.parametrize("name", ["efficientnet_b0", "efficientnet_b2", "efficientnet_b7"])
def test_state_dict_layout_matches_reference(name):
    from super_gradients_amd.training import models

    net = models.get(name, num_classes=10)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in _host_reference()["layouts"][name]]


def test_checkpoint_round_trip_with_reference_live():
    """Both directions, strictly, against the reference's own model class (needs the reference tree)."""
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine (the recorded state layout is checked by test_state_dict_layout_matches_reference)")
    from super_gradients_amd.training import models

    ref_shim.install()
    import super_gradients.training.models.classification_models.efficientnet as r
    from super_gradients.training.utils.utils import HpmStruct

    ref = r.EfficientNetB0(arch_params=HpmStruct(num_classes=10))
    G.deterministic_fill(ref, seed=9)
    net = models.get("efficientnet_b0", num_classes=10)
    net.load_state_dict(ref.state_dict(), strict=True)
    back = r.EfficientNetB0(arch_params=HpmStruct(num_classes=10))
    back.load_state_dict(net.state_dict(), strict=True)
    for (k, a), b in zip(ref.state_dict().items(), back.state_dict().values()):
        assert torch.equal(a, b), k


def test_initial_weight_distributions():
    """The reference initialises nothing itself: nn.Conv2d / nn.Linear defaults (kaiming_uniform with a = sqrt(5): U(-b, b), b = 1 / sqrt(fan_in),
    std b / sqrt(3); biases U(-b, b)), BatchNorm 1 / 0."""
    from super_gradients_amd.training import models

    sd = models.get("efficientnet_b0", num_classes=1000).state_dict()
    for key, fan_in in (("_conv_stem.weight", 27), ("_blocks.4._depthwise_conv.weight", 25), ("_blocks.5._expand_conv.weight", 40), ("_conv_head.weight", 320),
                        ("_blocks.15._se_reduce.weight", 1152), ("_blocks.15._se_expand.weight", 48), ("_fc.weight", 1280)):
        b = fan_in ** -0.5
        assert float(sd[key].abs().max()) <= b and abs(float(sd[key].std()) / (b / 3 ** 0.5) - 1.0) < 0.1, key
    for key, fan_in in (("_blocks.15._se_reduce.bias", 1152), ("_blocks.15._se_expand.bias", 48), ("_fc.bias", 1280)):
        assert 0 < float(sd[key].abs().max()) <= fan_in ** -0.5, key
    assert bool((sd["_blocks.5._bn1.weight"] == 1).all()) and bool((sd["_blocks.5._bn1.bias"] == 0).all())


def test_backbone_mode_and_its_load_rule(backend):
    from super_gradients_amd.training import models

    full = models.get("CustomizedEfficientnet", arch_params=dict(CUSTOM), num_classes=5)
    G.deterministic_fill(full, seed=2)
    back = models.get("CustomizedEfficientnet", arch_params=dict(CUSTOM, backbone_mode=True), num_classes=5)
    assert not any(k.startswith("_fc") for k in back.state_dict()) and list(back.state_dict()) == list(full.state_dict())[:-2]
    # the reference's rule: the last two entries are dropped and the 'module.' prefix removed; names without the prefix are an error
    back.load_state_dict({f"module.{k}": v for k, v in full.state_dict().items()}, strict=True)
    for k, v in back.state_dict().items():
        assert torch.equal(v, full.state_dict()[k]), k
    with pytest.raises(IndexError):
        back.load_state_dict(full.state_dict())
    back.materialize(backend).eval()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(backend)
    with torch.no_grad():
        feat = back(x)
    assert tuple(feat.shape) == (2, 640, 1, 1) and bool(torch.isfinite(feat.cpu()).all())


# --------------------------------------------------------------------------------------------- models
def _product_against_reference(name, device, fx, arch):
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    net = models.get(name, arch_params=dict(arch), num_classes=10)
    G.deterministic_fill(net, seed=4)
    net.materialize(device).train()
    x, y = fx["x"], fx["y"]
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_product_efficientnet_golden(gpu_device, name):
    x, y = _model_inputs()
    _product_against_reference(name, gpu_device, dict(_model_reference(name), x=x, y=y), ARCH)


def test_product_customized_efficientnet_emulation():
    """CustomizedEfficientnet (width 0.5, depth 0.3, res 32: 8 blocks) on the host emulation against the LIVE reference."""
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine (the chip runs efficientnet_b0 / _b2 against recorded tensors)")
    import emu_env

    ref_shim.install()
    import super_gradients.training.models.classification_models.efficientnet as r
    from super_gradients.training.utils.utils import HpmStruct

    ref = r.CustomizedEfficientnet(arch_params=HpmStruct(num_classes=10, backbone_mode=False, **CUSTOM))
    G.deterministic_fill(ref, seed=4)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)
    fx = dict(_run_reference(ref, x, y), x=x, y=y)
    emu_env.activate()
    try:
        _product_against_reference("CustomizedEfficientnet", torch.device("cpu"), fx, CUSTOM)
    finally:
        emu_env.deactivate()


# --------------------------------------------------------------------------------------------- trainer
@pytest.mark.gpu
def test_trainer_steps_efficientnet_b0(gpu_device, tmp_path):
    """Two Trainer steps of efficientnet_b0 at 8 x 3 x 32 x 32 with the ImageNet recipe's hyperparameters (RMSpropTF momentum 0.9, eps 1e-3,
    weight decay 1e-5; constant-decay EMA 0.9999; StepLRScheduler; label smoothing 0.1; the model's drop-connect 0.2 and dropout 0.2):
    finite loss, the parameters move, every BatchNorm counted two batches."""
    from super_gradients_amd.training import Trainer, models

    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(8, 3, 32, 32, generator=g), torch.arange(8) % 6
    loader = [(x, labels)] * 2
    torch.manual_seed(11)
    net = models.get("efficientnet_b0", arch_params=dict(image_size=32), num_classes=6)
    assert net.drop_connect_rate == 0.2 and net._dropout.p == 0.2
    before = {k: v.clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    tp = dict(max_epochs=1, lr_mode="StepLRScheduler", step_lr_update_freq=2.4, initial_lr=0.016, lr_decay_factor=0.97, optimizer="RMSpropTF",
              optimizer_params=dict(momentum=0.9, weight_decay=1e-5, eps=0.001), ema=True, ema_params=dict(decay=0.9999, decay_type="constant"),
              loss="CrossEntropyLoss", criterion_params=dict(smooth_eps=0.1), zero_weight_decay_on_bias_and_bn=True, average_best_models=False,
              metric_to_watch="Accuracy", greater_metric_to_watch_is_better=True, train_metrics_list=["Accuracy"], valid_metrics_list=["Accuracy"],
              silent_mode=True, seed=3)
    res = Trainer("effnet", ckpt_root_dir=str(tmp_path)).train(net, tp, loader, valid_loader=loader[:1])
    loss = res[-1]["train"]["CrossEntropyLoss"]
    assert loss == loss and abs(loss) < 1e4, res
    sd = net.state_dict()
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    moved = [k for k, v in before.items() if k.endswith("weight") and not torch.equal(v, sd[k].cpu())]
    assert len(moved) == sum(k.endswith("weight") for k in before), "parameters that did not change"
    assert all(bool(torch.isfinite(v.cpu()).all()) for v in sd.values() if v.dtype.is_floating_point)
