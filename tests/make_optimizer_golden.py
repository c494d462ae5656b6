"""TEST INFRASTRUCTURE ONLY: writes the fixture of tests/test_optimizers.py from the LIVE reference (needs the reference tree; run once, in
the build container, on the CPU):   python tests/make_optimizer_golden.py

  tests/golden/optimizers.pt   a synthetic "arena" (six tensors of mixed sizes, two of them without weight decay, one all zero; sizes that are
                               no multiples of 4 and slot boundaries inside a 1024-element reduction tile), eight steps of seeded gradients,
                               and what the reference's own RMSpropTF, Lion and Lamb classes make of them, once in fp32 and once in fp64, for
                               every option row of CASES: final parameters (both precisions), final fp32 states, the per-step fp32 parameters of
                               each optimizer's first row; for Lamb the per-step trust ratios |p| / |u| of both runs (formed here from the
                               reference's states and checked against the step the reference took); for Lion the smallest fp64 |u| each element
                               saw (the test leaves elements whose sign is within rounding of undecided out of its element-wise comparison).

Only data is stored.  Tests never import this file.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "golden", "optimizers.pt")

SIZES = [1100, 37, 64, 150, 70, 131]  # slot 0 fills reduction tile 0; tile 1 holds the end of slot 0, four whole slots and slot 5
NO_WD = [False, True, True, False, False, False]
ZERO = 4  # the all-zero tensor (weight decay on: Lamb's |p| = 0 branch)
LARGE = 3  # a tensor of large weights: |p| > |u|, so Lamb's trust_clip changes its ratio
STEPS = 8
LION_MARGIN = 1e-6  # |u| (fp64) below this at any step: the element's sign is within rounding of undecided (u is a sum of terms of size ~0.1)
LION_EXCLUDED_CAP = 0.01

# (name, optimizer, constructor arguments, gradient scale)
CASES = [
    ("rmsproptf_defaults", "RMSpropTF", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9), 1.0),
    ("rmsproptf_centered", "RMSpropTF", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, centered=True), 1.0),
    ("rmsproptf_decoupled_decay", "RMSpropTF", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, decoupled_decay=True), 1.0),
    ("rmsproptf_lr_outside_momentum", "RMSpropTF", dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, lr_in_momentum=False), 1.0),
    ("rmsproptf_no_momentum", "RMSpropTF", dict(lr=1e-2, weight_decay=1e-4, momentum=0.0), 1.0),
    ("lamb_defaults_clip_active", "Lamb", dict(lr=1e-2), 1.0),  # |g| ~ 39 > max_grad_norm 1
    ("lamb_trust_clip", "Lamb", dict(lr=1e-2, trust_clip=True), 1.0),
    ("lamb_always_adapt", "Lamb", dict(lr=1e-2, always_adapt=True), 1.0),
    ("lamb_no_grad_averaging", "Lamb", dict(lr=1e-2, grad_averaging=False), 1.0),
    ("lamb_clip_inactive", "Lamb", dict(lr=1e-2), 1e-3),  # |g| ~ 0.04 < 1
    ("lion_no_weight_decay", "Lion", dict(lr=1e-2), 1.0),
    ("lion_weight_decay", "Lion", dict(lr=1e-2, weight_decay=0.1), 1.0),
]


def reference_classes():
    from oracle import ref_shim

    ref_shim.install()
    from super_gradients.training.utils.optimizers.lamb import Lamb
    from super_gradients.training.utils.optimizers.lion import Lion
    from super_gradients.training.utils.optimizers.rmsprop_tf import RMSpropTF

    return {"RMSpropTF": RMSpropTF, "Lion": Lion, "Lamb": Lamb}


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.cat([torch.zeros(n) if i == ZERO else torch.randn(n, generator=g) * (3.0 if i == LARGE else 0.1) for i, n in enumerate(SIZES)])
    grads = torch.randn(STEPS, sum(SIZES), generator=g)
    return p0, grads


def run(cls, kwargs, p0, grads, dtype, optimizer):
    """The reference's class on one Parameter per tensor, in the two groups the arena optimizers form (no decay / decay)."""
    params = [torch.nn.Parameter(t.clone().to(dtype)) for t in p0.split(SIZES)]
    wd = kwargs.get("weight_decay", {"Lamb": 0.01}.get(optimizer, 0.0))
    kw = {k: v for k, v in kwargs.items() if k != "weight_decay"}
    groups = [{"params": [p for p, z in zip(params, NO_WD) if z], "weight_decay": 0.0}, {"params": [p for p, z in zip(params, NO_WD) if not z], "weight_decay": wd}]
    opt = cls(groups, **kw)
    per_step, trust, umin = [], [], torch.full((sum(SIZES),), float("inf"), dtype=torch.float64)
    for k in range(STEPS):
        for p, g in zip(params, grads[k].to(dtype).split(SIZES)):
            p.grad = g.clone()
        before = [p.detach().clone() for p in params]
        if optimizer == "Lion":  # u of this step, from the state the reference holds before it
            b1 = kw.get("betas", (0.9, 0.99))[0]
            u = torch.cat([(opt.state[p]["exp_avg"] if len(opt.state[p]) else torch.zeros_like(p)) * b1 + p.grad * (1 - b1) for p in params])
            umin = torch.minimum(umin, u.abs().double())
        opt.step()
        if optimizer == "Lamb":  # trust ratios of this step, formed from the reference's own states and checked against the step it took
            row = []
            for p, b, z in zip(params, before, NO_WD):
                grp = opt.param_groups[0 if z else 1]
                b1, b2 = grp["betas"]
                st = opt.state[p]
                u = (st["exp_avg"] / (1 - b1 ** grp["step"])) / (st["exp_avg_sq"].sqrt() / (1 - b2 ** grp["step"]) ** 0.5 + grp["eps"]) + grp["weight_decay"] * b
                t = torch.ones((), dtype=dtype)
                if grp["weight_decay"] != 0 or grp["always_adapt"]:
                    pn, un = b.norm(2.0), u.norm(2.0)
                    t = pn / un if (pn > 0 and un > 0) else t
                    t = torch.minimum(t, torch.ones((), dtype=dtype)) if grp["trust_clip"] else t
                tol = 1e-12 if dtype == torch.float64 else 1e-5
                assert torch.allclose(p.detach(), b - grp["lr"] * t * u, rtol=tol, atol=tol), "the trust ratio formed here is not the one the reference applied"
                row.append(t.double())
            trust.append(torch.stack(row))
        per_step.append(torch.cat([p.detach().clone() for p in params]))
    names = sorted({k for p in params for k, v in opt.state[p].items() if torch.is_tensor(v)})
    states = {k: torch.cat([opt.state[p][k] for p in params]) for k in names}
    return torch.stack(per_step), states, (torch.stack(trust) if trust else None), umin


def lion_ok(res32, res64, umin, lr):
    keep = umin >= LION_MARGIN
    tol = STEPS * 4 * 2.0 ** -24 * torch.maximum(res64.abs(), torch.tensor(lr, dtype=torch.float64))
    return float((~keep).double().mean()) <= LION_EXCLUDED_CAP and bool(((res32.double() - res64).abs() <= tol)[keep].all())


def main():
    import warnings

    warnings.filterwarnings("ignore")
    classes = reference_classes()
    seed = 0
    while True:  # draw seeds until the reference's own fp32-against-fp64 Lion comparison stays inside the cap for the stored inputs
        p0, grads = inputs(seed)
        ok = True
        for name, optimizer, kwargs, gscale in CASES:
            if optimizer == "Lion":
                s32, _, _, _ = run(classes[optimizer], kwargs, p0, grads * gscale, torch.float32, optimizer)
                s64, _, _, umin = run(classes[optimizer], kwargs, p0, grads * gscale, torch.float64, optimizer)
                ok = ok and lion_ok(s32[-1], s64[-1], umin, kwargs["lr"])
        if ok:
            break
        seed += 1
    out = {"sizes": SIZES, "no_wd": NO_WD, "steps": STEPS, "seed": seed, "p0": p0, "grads": grads, "lion_margin": LION_MARGIN, "cases": {}}
    first = set()
    for name, optimizer, kwargs, gscale in CASES:
        s32, st32, t32, _ = run(classes[optimizer], kwargs, p0, grads * gscale, torch.float32, optimizer)
        s64, _, t64, umin = run(classes[optimizer], kwargs, p0, grads * gscale, torch.float64, optimizer)
        case = {"optimizer": optimizer, "kwargs": kwargs, "grad_scale": gscale, "final32": s32[-1].clone(), "final64": s64[-1].clone(),
                "states32": {k: v.clone() for k, v in st32.items()}}
        if optimizer not in first:
            first.add(optimizer)
            case["per_step32"] = s32.clone()
        if optimizer == "Lamb":
            case["trust32"], case["trust64"] = t32, t64
        if optimizer == "Lion":
            case["umin64"] = umin
            assert lion_ok(s32[-1], s64[-1], umin, kwargs["lr"])
        out["cases"][name] = case
        print(f"{name}: |final32 - final64| max {float((s32[-1].double() - s64[-1]).abs().max()):.3e}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(out, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
