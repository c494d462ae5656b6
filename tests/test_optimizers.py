"""The arena optimizers beyond AdamW / SGD: Adam, RMSprop, RMSpropTF, Lion, Lamb (csrc/optim.hip, training/utils/optimizers.py).

Kernel level (`backend` = host emulation and the MI355X): RMSpropTF, Lion and Lamb against what the reference's own classes made of a
synthetic arena (tests/golden/optimizers.pt, written by tests/make_optimizer_golden.py); Adam and RMSprop live against torch.optim.
The bar is the project's three-way form: after eight steps each tensor's distance from the fp64 trajectory may be at most K times the fp32
reference's own distance from it, plus a floor of one ulp (ATen's CPU add(alpha=) may or may not fuse its multiply-add, so bit
equality with the fp32 reference is no property to demand).
Public interface: build_optimizer's seven names, recipe defaults, Trainer.train() against the same loop on torch.optim, checkpoint round
trips of the new state buffers, Lamb's adaptation under zero-weight-decay grouping, world size 2 over gloo."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from test_trainer import _loader, _tiny_models, no_op_kernels  # noqa: F401  (no_op_kernels: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "optimizers.pt")
GOLDEN_CASES = ["rmsproptf_defaults", "rmsproptf_centered", "rmsproptf_decoupled_decay", "rmsproptf_lr_outside_momentum", "rmsproptf_no_momentum",
                "lamb_defaults_clip_active", "lamb_trust_clip", "lamb_always_adapt", "lamb_no_grad_averaging", "lamb_clip_inactive",
                "lion_no_weight_decay", "lion_weight_decay"]
# Three-way factor k = (max|ours - fp64| - floor) / max|ref32 - fp64|, worst tensor of every row (the 12 fixture rows and the 6 live rows; the
# figures are in DESIGN.md 13.3).  Measured on the host emulation (no contraction, like ATen's unfused paths): 0.73.  The bar carries the 2x
# margin of the three-way checks in tests/test_yolo_nas.py.
K_THREE_WAY = 1.5
# Lamb's trust ratios against |p| / |u| in fp64: same form, same factor; floor = 2^-22 relative (the ratio of two fp32-rounded norms).
TRUST_FLOOR = 2.0 ** -22


def _fixture():
    return torch.load(FIXTURE)


def _tables(sizes, no_wd, wd, dev):
    """(seg_end, seg_wd) as optimizers._segments merges them, and the slot table."""
    ends, wds, slot_end, off = [], [], [], 0
    for n, z in zip(sizes, no_wd):
        off += n
        slot_end.append(off)
        w = 0.0 if z else float(wd)
        if wds and wds[-1] == w:
            ends[-1] = off
        else:
            ends.append(off)
            wds.append(w)
    return (torch.tensor(ends, dtype=torch.int64, device=dev), torch.tensor(wds, dtype=torch.float32, device=dev),
            torch.tensor(slot_end, dtype=torch.int64, device=dev))


class _ArenaRun:
    """One optimizer over a synthetic arena through the kernel wrappers (the arena classes themselves need an SgxNetwork, whose slots are
    64-element aligned: here slot boundaries fall anywhere)."""

    DEFAULTS = {
        "RMSpropTF": dict(lr=1e-2, alpha=0.9, eps=1e-10, weight_decay=0.0, momentum=0.0, centered=False, decoupled_decay=False, lr_in_momentum=True),
        "RMSprop": dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
        "Adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
        "Lion": dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0),
        "Lamb": dict(lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True, max_grad_norm=1.0, trust_clip=False,
                     always_adapt=False),
    }

    def __init__(self, optimizer, kwargs, p0, sizes, no_wd, dev):
        from super_gradients_amd import kernels as K

        self.K, self.name, self.h = K, optimizer, dict(self.DEFAULTS[optimizer], **kwargs)
        self.p = p0.clone().to(dev)
        n = self.p.numel()
        self.seg_end, self.seg_wd, self.slot_end = _tables(sizes, no_wd, self.h["weight_decay"], dev)
        z = lambda v=0.0: torch.full((n,), v, dtype=torch.float32, device=dev)  # noqa: E731
        h = self.h
        if optimizer in ("RMSprop", "RMSpropTF"):
            self.state = {"square_avg": z(1.0 if optimizer == "RMSpropTF" else 0.0), "grad_avg": z() if h["centered"] else None,
                          "momentum_buffer": z() if h["momentum"] > 0 else None}
        elif optimizer == "Lion":
            self.state = {"exp_avg": z()}
        else:
            self.state = {"exp_avg": z(), "exp_avg_sq": z()}
        if optimizer == "Lamb":
            self.ws = K.lamb_workspace(n, len(sizes), dev)
            self.trust = torch.zeros(len(sizes), dtype=torch.float32, device=dev)
        self.k = 0

    def step(self, g, grad_scale=None):
        K, h, s = self.K, self.h, self.state
        self.k += 1
        if self.name == "Adam":
            K.adam_step(self.p, g, s["exp_avg"], s["exp_avg_sq"], h["lr"], h["betas"][0], h["betas"][1], h["eps"], self.k, self.seg_end, self.seg_wd, grad_scale)
        elif self.name in ("RMSprop", "RMSpropTF"):
            K.rmsprop_step(self.p, g, s["square_avg"], s["grad_avg"], s["momentum_buffer"], h["lr"], h["alpha"], h["eps"], h["momentum"], self.seg_end,
                           self.seg_wd, tf=self.name == "RMSpropTF", decoupled_decay=h.get("decoupled_decay", False),
                           lr_in_momentum=h.get("lr_in_momentum", False), grad_scale=grad_scale)
        elif self.name == "Lion":
            K.lion_step(self.p, g, s["exp_avg"], h["lr"], h["betas"][0], h["betas"][1], self.seg_end, self.seg_wd, grad_scale)
        else:
            K.lamb_step(self.p, g, s["exp_avg"], s["exp_avg_sq"], h["lr"], h["betas"][0], h["betas"][1], h["eps"], self.k if h["bias_correction"] else 0,
                        self.seg_end, self.seg_wd, self.slot_end, self.ws, self.trust, grad_averaging=h["grad_averaging"], max_grad_norm=h["max_grad_norm"],
                        trust_clip=h["trust_clip"], always_adapt=h["always_adapt"], grad_scale=grad_scale)


def _three_way(name, ours, ref32, ref64, sizes, steps, lr):
    """Per tensor: max |ours - fp64| <= K * max |fp32 reference - fp64| + floor.  Prints every ratio before asserting.
    floor: ONE fp32 ulp of the tensor's largest weight (of lr, for the all-zero tensor) - for tensors where the fp32 reference happens to land
    on the rounded fp64 result and any other correct fp32 implementation is one rounding away."""
    bad, worst = [], 0.0
    for i, (o, a, b) in enumerate(zip(ours.double().split(sizes), ref32.double().split(sizes), ref64.split(sizes))):
        d_o, d_r = float((o - b).abs().max()), float((a - b).abs().max())
        floor = 2.0 ** -23 * max(float(b.abs().max()), lr)
        k = max(d_o - floor, 0.0) / max(d_r, 1e-300)
        worst = max(worst, k)
        print(f"three-way {name} tensor {i}: ours-fp64 {d_o:.3e} ref32-fp64 {d_r:.3e} floor {floor:.2e} k = (ours - floor) / ref32 = {k:.2f}")
        if d_o > K_THREE_WAY * d_r + floor:
            bad.append((i, d_o, d_r, floor))
    print(f"three-way {name}: worst k {worst:.2f}")
    assert not bad, f"{name}: (tensor, ours-fp64, ref32-fp64, floor) {bad}"


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_reference_trajectories(backend, case):
    """RMSpropTF / Lamb / Lion: eight steps against the reference's own classes (fixture), three-way; the final fp32 states against the
    reference's within the same bar's absolute size; Lamb's trust ratios of every step against |p| / |u| of the fp64 run."""
    fx = _fixture()
    c = fx["cases"][case]
    run = _ArenaRun(c["optimizer"], c["kwargs"], fx["p0"], fx["sizes"], fx["no_wd"], backend)
    grads = (fx["grads"] * c["grad_scale"]).to(backend)
    trust = []
    for k in range(fx["steps"]):
        run.step(grads[k].contiguous())
        if c["optimizer"] == "Lamb":
            trust.append(run.trust.cpu().clone())
    _three_way(case, run.p.cpu(), c["final32"], c["final64"], fx["sizes"], fx["steps"], run.h["lr"])
    for k, ref in c["states32"].items():
        if k == "step":
            continue
        got = run.state[k].cpu()
        scale = max(float(ref.abs().max()), 1e-30)
        e = float((got - ref).abs().max()) / scale
        print(f"state {case} {k}: max |ours - ref32| / max |ref32| = {e:.3e}")
        assert e <= 1e-5, f"{case}: state {k} differs from the reference's by {e:.2e} of its largest element"
    assert set(k for k, v in run.state.items() if v is not None) == set(c["states32"]) - {"step"}, "state buffers exist exactly for what is enabled"
    if c["optimizer"] == "Lamb":
        t, t32, t64 = torch.stack(trust).double(), c["trust32"], c["trust64"]
        d_o, d_r = (t - t64).abs() / t64, (t32 - t64).abs() / t64
        print(f"trust {case}: ours-fp64 max {float(d_o.max()):.3e} ref32-fp64 max {float(d_r.max()):.3e}; last step {t[-1].tolist()}")
        assert bool((d_o <= K_THREE_WAY * d_r.max() + TRUST_FLOOR).all()), f"{case}: trust ratios {float(d_o.max()):.3e} from fp64 (fp32 reference {float(d_r.max()):.3e})"
        zero, no_wd = 4, [i for i, z in enumerate(fx["no_wd"]) if z]
        assert float(t[0, zero]) == 1.0, "|p| = 0: trust ratio 1"
        if not c["kwargs"].get("always_adapt"):
            assert bool((t[:, no_wd] == 1.0).all()), "no adaptation on tensors without weight decay"
        else:
            assert bool((t[:, no_wd] != 1.0).all())
        if c["kwargs"].get("trust_clip"):
            assert float(t.max()) <= 1.0 and float(c["trust64"].max()) == 1.0  # (the fixture has a tensor whose unclipped ratio is above 1)


LIVE_ROWS = {
    "adam_weight_decay": ("Adam", dict(lr=1e-2, weight_decay=1e-4)),
    "adam_betas_eps": ("Adam", dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6)),
    "rmsprop_momentum": ("RMSprop", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9)),
    "rmsprop_centered_momentum": ("RMSprop", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, centered=True)),
    "rmsprop_plain": ("RMSprop", dict(lr=1e-2)),
    "rmsprop_centered": ("RMSprop", dict(lr=1e-2, alpha=0.9, centered=True)),
}


@pytest.mark.parametrize("row", list(LIVE_ROWS))
def test_adam_rmsprop_against_torch(backend, row):
    """Adam / RMSprop live against torch.optim on the same synthetic arena, fp32 and fp64, three-way."""
    fx = _fixture()
    name, kwargs = LIVE_ROWS[row]
    sizes, no_wd, steps = fx["sizes"], fx["no_wd"], fx["steps"]

    def torch_run(dtype):
        params = [torch.nn.Parameter(t.clone().to(dtype)) for t in fx["p0"].split(sizes)]
        kw = {k: v for k, v in kwargs.items() if k != "weight_decay"}
        groups = [{"params": [p for p, z in zip(params, no_wd) if z], "weight_decay": 0.0},
                  {"params": [p for p, z in zip(params, no_wd) if not z], "weight_decay": kwargs.get("weight_decay", 0.0)}]
        o = (torch.optim.Adam if name == "Adam" else torch.optim.RMSprop)(groups, **kw)
        for k in range(steps):
            for p, g in zip(params, fx["grads"][k].to(dtype).split(sizes)):
                p.grad = g.clone()
            o.step()
        return torch.cat([p.detach() for p in params])

    run = _ArenaRun(name, kwargs, fx["p0"], sizes, no_wd, backend)
    for k in range(steps):
        run.step(fx["grads"][k].to(backend).contiguous())
    _three_way(row, run.p.cpu(), torch_run(torch.float32), torch_run(torch.float64), sizes, steps, run.h["lr"])
    assert (run.state.get("grad_avg") is not None) == bool(kwargs.get("centered")) or name == "Adam"


@pytest.mark.parametrize("case", ["lion_no_weight_decay", "lion_weight_decay"])
def test_lion_elementwise(backend, case):
    """Element-wise, a few ulp per step: 4 ulp x 8 steps of max(|p|, lr).  A wrong sign is a 2 lr = 2e-2 error, 1e4 times the tolerance.
    Elements whose fp64 |u| came within 1e-6 of zero at any step (u is a sum of two terms of size ~0.1 - 1: 1e-6 is ~10 ulp of them) may
    legitimately flip between two fp32 implementations and are left out; they may be at most 1 % of the elements."""
    fx = _fixture()
    c = fx["cases"][case]
    run = _ArenaRun("Lion", c["kwargs"], fx["p0"], fx["sizes"], fx["no_wd"], backend)
    for k in range(fx["steps"]):
        run.step(fx["grads"][k].to(backend).contiguous())
    keep = c["umin64"] >= 1e-6
    excluded = float((~keep).double().mean())
    print(f"lion {case}: excluded share {excluded:.4%}")
    assert excluded <= 0.01
    tol = fx["steps"] * 4 * 2.0 ** -24 * torch.maximum(c["final64"].abs(), torch.tensor(run.h["lr"], dtype=torch.float64))
    err = (run.p.cpu().double() - c["final64"]).abs()
    print(f"lion {case}: max err / tol on kept elements {float((err / tol)[keep].max()):.3f}")
    assert bool((err <= tol)[keep].all()), f"{int((err > tol)[keep].sum())} elements off, worst {float(err[keep].max()):.3e}"
    e = float((run.state["exp_avg"].cpu() - c["states32"]["exp_avg"]).abs().max())
    assert e <= 8 * 2.0 ** -23 * float(c["states32"]["exp_avg"].abs().max())


def test_lion_known_answer(backend):
    """Powers of two, every intermediate exact: lr 2^-3, wd 2 -> decay factor 3/4; betas (1/2, 1/4).
    Order pinned: decay FIRST (p 1 -> 3/4), sign of u = m/2 + g/2 from the OLD m, then m = m/4 + 3g/4.  Element 2: u = 0 exactly -> no step.
    Element 3: m and g of opposite sign with |m| > |g|: the sign follows m (a step taken after the momentum update would follow g)."""
    from super_gradients_amd import kernels as K

    dev = backend
    p = torch.tensor([1.0, -2.0, 4.0, 1.0, 8.0, -1.0, 2.0, 0.5, 16.0], device=dev)
    m = torch.tensor([0.5, 0.25, 1.0, -1.0, 0.0, 0.0, -4.0, 2.0, 0.0], device=dev)
    g = torch.tensor([0.5, -1.0, -1.0, 0.5, 2.0, -0.25, 8.0, -2.0, 0.0], device=dev)
    seg_end = torch.tensor([8, 9], dtype=torch.int64, device=dev)
    seg_wd = torch.tensor([2.0, 0.0], device=dev)  # the last element: no decay
    K.lion_step(p, g, m, 0.125, 0.5, 0.25, seg_end, seg_wd)
    u = [0.5, -0.375, 0.0, -0.25, 1.0, -0.125, 2.0, 0.0, 0.0]
    exp_p = [pi * (0.75 if i < 8 else 1.0) - 0.125 * float(np.sign(ui)) for i, (pi, ui) in enumerate(zip([1.0, -2.0, 4.0, 1.0, 8.0, -1.0, 2.0, 0.5, 16.0], u))]
    exp_m = [0.25 * mi + 0.75 * gi for mi, gi in zip([0.5, 0.25, 1.0, -1.0, 0.0, 0.0, -4.0, 2.0, 0.0], [0.5, -1.0, -1.0, 0.5, 2.0, -0.25, 8.0, -2.0, 0.0])]
    assert p.cpu().tolist() == exp_p, (p.cpu().tolist(), exp_p)
    assert m.cpu().tolist() == exp_m, (m.cpu().tolist(), exp_m)


def test_lamb_is_deterministic(backend):
    """Identical inputs -> bit-identical parameters, moments and trust ratios (fixed-order fp64 folds, no atomics), a handful of repeats.  The
    launch geometry is not configurable, and the partial sums belong to tiles of the arena, not to workgroups: a second arena size changes
    the grid (one tile, a partly filled last tile) and is checked the same way."""
    fx = _fixture()
    for cut in (None, 1000, 1301):
        sizes, no_wd = fx["sizes"], fx["no_wd"]
        if cut is not None:
            sizes, no_wd = ([cut], [False]) if cut <= sizes[0] else ([sizes[0], 37, 64, cut - sizes[0] - 101], no_wd[:4])
        n = sum(sizes)
        outs = []
        for rep in range(4):
            run = _ArenaRun("Lamb", dict(lr=1e-2), fx["p0"][:n], sizes, no_wd, backend)
            for k in range(2):
                run.step(fx["grads"][k][:n].to(backend).contiguous())
            outs.append((run.p.cpu().clone(), run.trust.cpu().clone(), run.state["exp_avg_sq"].cpu().clone()))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0])), f"arena of {n}: two runs differ"


def test_lamb_grad_scale_is_the_mean_gradient(backend):
    """grad_scale folds the data-parallel mean in: the step over (2 g, grad_scale 1/2) equals the step over g bit for bit - norms, clip factor
    and moments all see the mean gradient.  max_grad_norm sits between |g| and |2 g|: a clip taken of the sum would be active."""
    fx = _fixture()
    g = (fx["grads"][0] * 1e-3).to(backend).contiguous()
    gn = float(g.double().norm())
    kw = dict(lr=1e-2, max_grad_norm=1.5 * gn, eps=1e-3)
    a = _ArenaRun("Lamb", kw, fx["p0"], fx["sizes"], fx["no_wd"], backend)
    b = _ArenaRun("Lamb", kw, fx["p0"], fx["sizes"], fx["no_wd"], backend)
    a.step(g)
    b.step((g * 2).contiguous(), grad_scale=torch.tensor([0.5], device=backend))
    assert torch.equal(a.p.cpu(), b.p.cpu()) and torch.equal(a.trust.cpu(), b.trust.cpu())
    g_before = g.clone()
    a.step(g)
    assert torch.equal(g, g_before), "the gradient arena is not written"


# ------------------------------------------------------------------------------------------------ public interface
def test_build_optimizer_resolves_the_reference_names(no_op_kernels):
    """The registry's seven names (optimizer_utils.py:88-143), any letter case; an unknown name lists what exists."""
    from super_gradients_amd.common.registry import OPTIMIZERS as REGISTRY
    from super_gradients_amd.training.utils import optimizers as O
    from super_gradients_amd.training.utils.utils import HpmStruct

    _, net = _tiny_models(no_op_kernels)
    net.materialize(no_op_kernels)
    expect = {"SGD": O.ArenaSGD, "Adam": O.ArenaAdam, "AdamW": O.ArenaAdamW, "RMSprop": O.ArenaRMSprop, "RMSpropTF": O.ArenaRMSpropTF, "Lamb": O.ArenaLamb,
              "Lion": O.ArenaLion}
    for name, cls in expect.items():
        for spelled in (name, name.lower(), name.upper()):
            opt = O.build_optimizer(net, 0.1, HpmStruct(optimizer=spelled, optimizer_params={}, zero_weight_decay_on_bias_and_bn=True))
            assert type(opt) is cls and opt.param_groups[0]["lr"] == 0.1
            assert [g["name"] for g in opt.param_groups] == ["no_decay", "decay"] and opt.param_groups[0]["weight_decay"] == 0.0
        assert REGISTRY[name] is cls
    with pytest.raises(NotImplementedError, match="Lamb.*Lion|Lion.*Lamb"):
        O.build_optimizer(net, 0.1, HpmStruct(optimizer="Adagrad", optimizer_params={}))
    # constructor defaults and argument checks of the reference's classes
    lamb = O.ArenaLamb(net)
    assert (lamb.defaults["eps"], lamb.defaults["weight_decay"], lamb.defaults["max_grad_norm"], lamb.defaults["lr"]) == (1e-6, 0.01, 1.0, 1e-3)
    lion = O.ArenaLion(net)
    assert (lion.defaults["lr"], lion.defaults["betas"], lion.defaults["weight_decay"]) == (1e-4, (0.9, 0.99), 0.0) and lion.state_names == ("exp_avg",)
    tf = O.ArenaRMSpropTF(net)
    assert (tf.defaults["alpha"], tf.defaults["eps"], tf.defaults["lr_in_momentum"], tf.defaults["decoupled_decay"]) == (0.9, 1e-10, True, False)
    assert tf.grad_avg is None and tf.momentum_buffer is None and float(tf.square_avg.min()) == 1.0
    assert O.ArenaRMSprop(net, momentum=0.9, centered=True).grad_avg is not None and float(O.ArenaRMSprop(net).square_avg.max()) == 0.0
    with pytest.raises(ValueError, match="Invalid learning rate"):
        O.ArenaLion(net, lr=-1.0)
    with pytest.raises(ValueError, match="Invalid beta parameter at index 1"):
        O.ArenaLion(net, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="Invalid alpha value"):
        O.ArenaRMSpropTF(net, alpha=-0.1)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        O.ArenaAdam(net, amsgrad=True)
    assert O.ArenaSGD.takes_grad_scale is False and all(c.takes_grad_scale for n, c in expect.items() if n != "SGD")


def test_reference_optimizer_params_defaults_adam_rmsprop(no_op_kernels):
    """The other half of tests/unit_tests/optimizer_params_override_test.py:9-70 (test_trainer.py has SGD's): Adam's recipe default weight
    decay 1e-4, RMSprop's and RMSpropTF's weight decay 1e-4 and momentum 0.9 (training/params.py:90-94) sit under the recipe's
    `optimizer_params`, and the merged dictionary is written back."""
    from super_gradients_amd.training.utils.optimizers import build_optimizer
    from super_gradients_amd.training.utils.utils import HpmStruct

    _, net = _tiny_models(no_op_kernels)
    net.materialize(no_op_kernels)
    tp = HpmStruct(optimizer="Adam", optimizer_params={}, zero_weight_decay_on_bias_and_bn=False)
    opt = build_optimizer(net, 0.1, tp)
    assert opt.defaults["weight_decay"] == 1e-4 and tp.optimizer_params == {"weight_decay": 1e-4}
    tp = HpmStruct(optimizer="Adam", optimizer_params={"weight_decay": 0.2}, zero_weight_decay_on_bias_and_bn=True)
    assert build_optimizer(net, 0.1, tp).defaults["weight_decay"] == 0.2 and tp.optimizer_params == {"weight_decay": 0.2}
    for name in ("RMSprop", "RMSpropTF"):
        tp = HpmStruct(optimizer=name, optimizer_params={}, zero_weight_decay_on_bias_and_bn=False)
        opt = build_optimizer(net, 0.1, tp)
        assert opt.defaults["momentum"] == 0.9 and opt.defaults["weight_decay"] == 1e-4 and tp.optimizer_params == {"weight_decay": 1e-4, "momentum": 0.9}
        assert opt.momentum_buffer is not None
        tp = HpmStruct(optimizer=name, optimizer_params={"momentum": 0.8, "alpha": 0.95}, zero_weight_decay_on_bias_and_bn=True)
        opt = build_optimizer(net, 0.1, tp)
        assert tp.optimizer_params == {"weight_decay": 1e-4, "momentum": 0.8, "alpha": 0.95} and opt.defaults["alpha"] == 0.95
    for name, wd in (("Lamb", 0.01), ("Lion", 0.0)):  # no recipe defaults: the classes' own apply
        tp = HpmStruct(optimizer=name, optimizer_params={}, zero_weight_decay_on_bias_and_bn=False)
        assert build_optimizer(net, 0.1, tp).defaults["weight_decay"] == wd and tp.optimizer_params == {}


@pytest.mark.parametrize("opt", ["Adam", "RMSprop"])
def test_trainer_matches_torch_loop_new_optimizers(backend, tmp_path, opt):
    """test_trainer.test_trainer_matches_torch_loop with optimizer="Adam" / "RMSprop": the same tiny conv network, the same loop written
    with torch.optim, the tolerances that test holds AdamW to."""
    from super_gradients_amd.training import Trainer
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.callbacks import CosineLRScheduler

    ref, net = _tiny_models(backend)
    n, epochs, bs = (3, 2, 4) if backend.type == "cuda" else (2, 2, 2)
    loader = _loader(n, bs, 1)
    initial_lr, warm_steps, warm_lr, ratio = (0.05, 2, 1e-3, 0.1) if opt == "Adam" else (0.01, 2, 1e-3, 0.1)
    oparams = dict(weight_decay=1e-2, betas=(0.9, 0.99)) if opt == "Adam" else dict(weight_decay=1e-2, momentum=0.9, alpha=0.9, eps=1e-3)
    tp = dict(max_epochs=epochs, lr_mode="CosineLRScheduler", initial_lr=initial_lr, loss=CrossEntropyLoss(), optimizer=opt, optimizer_params=oparams,
              zero_weight_decay_on_bias_and_bn=True, warmup_mode="LinearBatchLRWarmup", lr_warmup_steps=warm_steps, warmup_initial_lr=warm_lr,
              cosine_final_lr_ratio=ratio, silent_mode=True, seed=7, valid_metrics_list=["Accuracy"], metric_to_watch="Accuracy")
    res = Trainer("tiny_" + opt, ckpt_root_dir=str(tmp_path)).train(net, tp, loader, valid_loader=loader)
    decay = [p for _, p in ref.named_parameters() if p.dim() > 1]
    no_decay = [p for _, p in ref.named_parameters() if p.dim() <= 1]
    groups = [{"params": no_decay, "weight_decay": 0.0}, {"params": decay}]
    o = torch.optim.Adam(groups, lr=initial_lr, **oparams) if opt == "Adam" else torch.optim.RMSprop(groups, lr=initial_lr, **oparams)
    ref.train()
    losses = []
    for epoch in range(epochs):
        tot = 0.0
        for b, (x, y) in enumerate(loader):
            g = b + epoch * n
            if g < warm_steps:
                for pg in o.param_groups:
                    pg["lr"] = float(np.linspace(warm_lr, initial_lr, warm_steps)[g])
            loss = F.cross_entropy(ref(x), y)
            loss.backward()
            o.step()
            o.zero_grad()
            if g >= warm_steps:
                lr = float(CosineLRScheduler.compute_learning_rate(max(0, g - warm_steps), n * epochs - warm_steps, initial_lr, ratio))
                for pg in o.param_groups:
                    pg["lr"] = lr
            tot += float(loss) * bs
        losses.append(tot / (n * bs))
    for r, l in zip(res, losses):
        assert abs(r["train"]["CrossEntropyLoss"] - l) <= 2e-4 * abs(l), (r, l)
    sd = net.state_dict()
    for k, v in ref.state_dict().items():
        if v.dtype.is_floating_point:
            e = float((sd[k].cpu() - v).abs().max()) / max(float(v.abs().max()), 1e-3)
            print(f"trainer {opt} {k}: {e:.2e}")
            assert e <= 5e-4, f"{k}: {e:.2e}"


@pytest.mark.parametrize("opt", ["RMSpropTF", "Lamb"])
def test_trainer_resume_new_state_buffers(backend, tmp_path, opt):
    """tests/test_api.py::test_trainer_resume for the optimizers whose state the three hard-coded names did not cover: one epoch + a resumed
    second one == two epochs in one go.  RMSpropTF centered with momentum carries square_avg, grad_avg and momentum_buffer; Lamb carries
    exp_avg, exp_avg_sq and the step count its bias correction reads."""
    from super_gradients_amd.training import Trainer
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.callbacks import Callback

    loader = _loader(2, 2, 1)
    oparams = dict(momentum=0.9, centered=True, weight_decay=1e-3) if opt == "RMSpropTF" else dict(weight_decay=1e-2)

    def params(epochs, **kw):
        return dict(max_epochs=epochs, lr_mode="StepLRScheduler", lr_updates=[1], lr_decay_factor=0.5, initial_lr=0.01, loss=CrossEntropyLoss(), optimizer=opt,
                    optimizer_params=dict(oparams), zero_weight_decay_on_bias_and_bn=True, silent_mode=True, **kw)

    class StopAfterFirst(Callback):
        def on_train_loader_end(self, context):
            context.stop_training = True

    _, net_a = _tiny_models(backend)
    Trainer("a", ckpt_root_dir=str(tmp_path)).train(net_a, params(2), loader)
    _, net_b = _tiny_models(backend)
    Trainer("b", ckpt_root_dir=str(tmp_path)).train(net_b, params(2, phase_callbacks=[StopAfterFirst()]), loader)
    ckpt = torch.load(os.path.join(str(tmp_path), "b", "ckpt_latest.pth"))["optimizer_state_dict"]
    expect = {"square_avg", "grad_avg", "momentum_buffer"} if opt == "RMSpropTF" else {"exp_avg", "exp_avg_sq"}
    assert expect <= set(ckpt) and ckpt["steps"] == 2
    _, net_c = _tiny_models(backend)
    tr = Trainer("c", ckpt_root_dir=str(tmp_path))
    tr.train(net_c, params(2, resume_path=os.path.join(str(tmp_path), "b", "ckpt_latest.pth")), loader)
    assert tr.optimizer._steps == 4
    for (k, va), vc in zip(net_a.state_dict().items(), net_c.state_dict().values()):
        if va.dtype.is_floating_point:
            assert torch.allclose(va.cpu(), vc.cpu(), rtol=1e-5, atol=1e-6), k
    assert not torch.allclose(net_a.p_arena.buf.cpu(), net_b.p_arena.buf.cpu(), rtol=1e-5, atol=1e-6), "the second epoch moved the weights"


def test_checkpoint_state_names_of_adamw_and_sgd_are_unchanged(no_op_kernels):
    """Checkpoints written by AdamW / SGD stay compatible in both directions: the declared state names are the keys they always carried."""
    from super_gradients_amd.training.sg_trainer.sg_trainer import _optimizer_state_names
    from super_gradients_amd.training.utils import optimizers as O

    _, net = _tiny_models(no_op_kernels)
    net.materialize(no_op_kernels)
    assert _optimizer_state_names(O.ArenaAdamW(net)) == ("exp_avg", "exp_avg_sq") and _optimizer_state_names(O.ArenaSGD(net)) == ("momentum_buffer",)
    assert _optimizer_state_names(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)) == ("exp_avg", "exp_avg_sq", "momentum_buffer")


def test_lamb_skips_adaptation_on_bn_and_bias(backend):
    """zero_weight_decay_on_bias_and_bn: the trust ratio stays 1 exactly on the BatchNorm and bias slots and is |p| / |u| elsewhere; without
    the grouping every slot adapts (weight decay everywhere)."""
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaLamb

    for zero in (True, False):
        _, net = _tiny_models(backend)
        net.materialize(backend).train()
        opt = ArenaLamb(net, lr=1e-2, zero_weight_decay_on_bias_and_bn=zero)
        x, y = _loader(1, 4, 3)[0]
        CrossEntropyLoss()(net(x.to(backend)), y.to(backend)).backward()
        p0 = net.p_arena.buf.detach().cpu().double().clone()
        opt.step()
        trust = opt.trust.cpu()
        ends = opt.slot_end.cpu().tolist()
        assert len(ends) == len(net.slots) and any(s.no_wd for s in net.slots)
        for i, s in enumerate(net.slots):
            if (zero and s.no_wd) or float(p0[s.start:ends[i]].norm()) == 0.0:  # (BatchNorm biases start at zero: |p| = 0, ratio 1)
                assert float(trust[i]) == 1.0, s.name
            else:
                assert float(trust[i]) != 1.0 and math.isfinite(float(trust[i])), s.name
        # the ratio is |p| / |u| of the slot: recover |u| from the step taken, lr * trust * u = p0 - p1
        p1 = net.p_arena.buf.detach().cpu().double()
        for i, s in enumerate(net.slots):
            if not (zero and s.no_wd) and float(trust[i]) != 1.0:
                lo, hi = s.start, ends[i]
                un = float((p0[lo:hi] - p1[lo:hi]).norm()) / (1e-2 * float(trust[i]))
                assert abs(float(trust[i]) - float(p0[lo:hi].norm()) / un) <= 1e-4 * float(trust[i]), s.name


# ------------------------------------------------------------------------------------------------ world size 2 on gloo
def _worker_lamb(rank, world, port, outdir):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "emu"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import emu_env

    emu_env.activate()
    import torch.distributed as dist

    from super_gradients_amd.training.utils import distributed_training_utils as DU
    from super_gradients_amd.training.utils.distributed_training_utils import GradientAllReducer, setup_device_from_env
    from super_gradients_amd.training.utils.optimizers import ArenaLamb

    _, _, dev = setup_device_from_env(backend="gloo")
    gfull = torch.Generator().manual_seed(77)
    xfull, wfull = torch.randn(8, 4, 8, 8, generator=gfull), torch.randn(8, 6, generator=gfull)
    out = {}
    _, net = _tiny_models(dev)  # identical weights on both ranks (seeded inside)
    net.materialize(dev).train()
    net.set_sync_bn(True)
    reducer = GradientAllReducer(net, net.gradient_buckets())
    net.zero_grad()
    (net(xfull[rank * 4:(rank + 1) * 4]) * wfull[rank * 4:(rank + 1) * 4]).sum().backward()  # the arena now holds the SUM over ranks
    gsum = float(net.g_arena.buf.double().norm())
    # max_grad_norm between |mean gradient| and |summed gradient|, eps large enough for the update to feel the gradient's scale: a step taken
    # of the sum (its norm, or its moments) lands elsewhere
    kw = dict(lr=1e-2, eps=1e-2, max_grad_norm=0.75 * gsum, zero_weight_decay_on_bias_and_bn=True)
    out["max_grad_norm"], out["p0"] = kw["max_grad_norm"], net.p_arena.buf.clone()
    opt = ArenaLamb(net, **kw)
    opt.step(grad_scale=reducer.grad_scale)
    out["params"], out["trust"] = net.p_arena.buf.clone(), opt.trust.clone()
    if rank == 0:  # one process, the concatenated batch, the mean loss
        _, one = _tiny_models(dev)
        one.materialize(dev).train()
        one.zero_grad()
        (one(xfull) * wfull * 0.5).sum().backward()
        out["gmean"] = float(one.g_arena.buf.double().norm())
        o1 = ArenaLamb(one, **kw)
        o1.step()
        out["single"], out["single_trust"] = one.p_arena.buf.clone(), o1.trust.clone()
        # the same single-process step fed the SUM: what a step that ignored the mean would give
        _, two = _tiny_models(dev)
        two.materialize(dev).train()
        two.zero_grad()
        (two(xfull) * wfull).sum().backward()
        ArenaLamb(two, **kw).step()
        out["of_sum"] = two.p_arena.buf.clone()
    torch.save(out, os.path.join(outdir, f"lamb{rank}.pt"))
    DU.barrier()
    dist.destroy_process_group()


def test_world_size_2_gloo_lamb(tmp_path):
    """Lamb under data parallelism (gloo, host emulation, the form of tests/test_distributed.py): both ranks end with identical parameters,
    equal to a single-process step on the concatenated batch - so clip factor, moments and per-slot norms are those of the MEAN gradient.
    Tolerance: tests/test_distributed.py has no AdamW comparison; its bar for the quantity that differs here - the synchronised-BatchNorm
    gradient of two half batches against the full batch - is 2e-4 of the largest element, and that is applied to the step taken."""
    world = 2
    port = 30100 + (os.getpid() % 2000)
    mp.spawn(_worker_lamb, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"lamb{i}.pt")) for i in range(world)]
    assert torch.equal(r[0]["params"], r[1]["params"]) and torch.equal(r[0]["trust"], r[1]["trust"])
    assert r[0]["gmean"] < r[0]["max_grad_norm"] < 2 * r[0]["gmean"], "the clip threshold separates the mean gradient from the sum"
    step = (r[0]["single"] - r[0]["p0"]).abs().max()
    e = float((r[0]["params"] - r[0]["single"]).abs().max() / step)
    e_sum = float((r[0]["of_sum"] - r[0]["single"]).abs().max() / step)
    print(f"lamb world 2: |dp - single| / step {e:.2e}; a step of the summed gradient would be {e_sum:.2e} away")
    assert e <= 2e-4, e
    assert e_sum > 100 * 2e-4, "the check would not notice a step taken of the summed gradient"
    assert torch.allclose(r[0]["trust"], r[0]["single_trust"], rtol=2e-4)
