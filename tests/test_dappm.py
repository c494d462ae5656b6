"""The DAPPM module (segmentation_models/ddrnet.py) against the reference's own DAPPM run in fp64.

  reference (through the import shim)  ->  recorded tensors   CPU: live where the reference tree exists, tests/golden/dappm_reference.pt elsewhere
      (tests/make_dappm_golden.py writes it)
  product (HIP kernels; `backend`: the host emulation of the same kernel sources, or the chip)  <-  those recorded tensors
Bar: the module-level one, 1e-4 of each tensor's largest element, for the training forward, the input gradient, every parameter gradient, the
running statistics after the step and the eval forward.  The seeds are chosen so that no BatchNorm -> ReLU pre-activation of the fp64 run lies
within 1e-5 of zero (a ReLU mask cannot flip inside the bar); the fixture records each map's minimum and the test asserts it."""
import pytest
import torch

from oracle import golden_util as G
from oracle import ref_shim
from test_mobilenet import _check_grads, _wrap
from util import assert_close, to_nchw_cpu, to_nhwc

ARGS = (16, 8, 16, [1, 5, 9, 17, 0], [1, 2, 4, 8, 0])
SHAPES = {"10x12": (2, 16, 10, 12), "16x32": (2, 16, 16, 32)}  # 10 / 3: the 9 / 4 / 4 level is 3 rows high - no integer scale


def _reference():
    def compute():
        ref_shim.install()
        from super_gradients.training.models.segmentation_models.ddrnet import DAPPM as RefDAPPM

        out = {}
        for i, (name, shape) in enumerate(SHAPES.items()):
            mod = RefDAPPM(*ARGS)
            G.deterministic_fill(mod, seed=21 + i)
            state = {k: v.clone() for k, v in mod.state_dict().items()}
            mod.double().train()
            g = torch.Generator().manual_seed(3 + i)
            x = torch.randn(shape, generator=g) + 0.5
            pre = []
            hooks = [m.register_forward_hook(lambda m, a, o: pre.append(float(o.detach().abs().min()))) for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d)]
            xa = x.double().requires_grad_(True)
            y = mod(xa)
            for h in hooks:
                h.remove()
            dy = torch.randn(y.shape, generator=g)
            y.backward(dy.double())
            rec = dict(state=state, x=x, y=y.detach().float(), dy=dy, x_grad=xa.grad.float(), min_preact=torch.tensor(pre),
                       grads={k: p.grad.float() for k, p in mod.named_parameters()},
                       buffers={k: v.float() for k, v in mod.named_buffers() if not k.endswith("num_batches_tracked")})
            if name == "10x12":  # (the eval forward is checked at one shape)
                mod.eval()
                with torch.no_grad():
                    rec["y_eval"] = mod(x.double()).float()
            out[name] = rec
        return out

    return G.reference_outputs("dappm_reference", compute)


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_dappm_against_reference(backend, cfg):
    from super_gradients_amd.training.models.segmentation_models import DAPPM

    fx = _reference()[cfg]
    assert fx["min_preact"].numel() == 11 and float(fx["min_preact"].min()) > 1e-5
    blk = DAPPM(*ARGS)
    assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == [(k, tuple(v.shape)) for k, v in fx["state"].items()]
    net = _wrap([blk], backend)
    net.load_state_dict({f"0.{k}": v for k, v in fx["state"].items()}, strict=True)
    net.train()
    net.zero_grad()
    y = blk.fwd(to_nhwc(fx["x"], backend))
    assert_close(to_nchw_cpu(y), fx["y"], 1e-4, "training forward")
    dx = blk.bwd(to_nhwc(fx["dy"], backend))
    net.join_side()
    assert_close(to_nchw_cpu(dx), fx["x_grad"], 1e-4, "input gradient")
    _check_grads(blk, fx, 1e-4)
    for k, b in blk.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(b.cpu(), fx["buffers"][k], 1e-4, k)
    if cfg == "10x12":  # eval mode, on the running statistics the step left
        net.eval()
        with torch.no_grad():
            assert_close(to_nchw_cpu(blk.fwd(to_nhwc(fx["x"], backend))), fx["y_eval"], 1e-4, "eval forward")


def test_refusals():
    from super_gradients_amd.training.models.segmentation_models import DAPPM

    with pytest.raises(NotImplementedError):
        DAPPM(16, 8, 16, [1, 5, 0], [1, 2, 0], inter_mode="nearest")
    with pytest.raises(NotImplementedError):
        DAPPM(16, 8, 16, [1, 19, 0], [1, 8, 0])
