"""Bit parity of the row-by-channel sweeps (csrc/bn.hip) between two builds of the library.

    python tools/sweep_parity.py record FILE.npz [--backend gpu|emu]     on the build that is the yardstick (the parent commit)
    python tools/sweep_parity.py check  FILE.npz [--backend gpu|emu]     on the build under test: every array must have the same bits

Copy this file into the yardstick's tools/ directory to record there: it calls only `kernels` wrappers that every build has (tri_affine_act,
tri_affine_act_bwd_reduce - its one-branch form only where the build has it -, affine_act, bn_bwd, axpy, relu_bwd, relu_bwd_bn_reduce, channel_stats_partial, qarep_bwd,
colsum).  FILE belongs outside the repository's history (a job's output directory).
Cases: the seeded inputs of tests/test_repvgg_kernels.py (`_case`) on (3, 23, 19, c) for c = 4 (one channel group, most row lanes idle), 48 (a
row-lane count that does not divide 256), 96 (the unrolled loop and its tail), 260 (two channel strips, the second with one live group), and
(2, 7, 7, 1280) (five strips); strided operands and outputs; every activation a kernel takes; the statistics rows on and off; the default
row blocks, 3 and one row per block where the entry point takes a block count.  Recorded: the logical outputs and the partial rows.
`--backend emu` runs the host emulation of the same sources (tests/emu)."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, 23, 19, 4), (3, 23, 19, 48), (3, 23, 19, 96), (3, 23, 19, 260), (2, 7, 7, 1280)]
ACTS3 = (None, "relu", "silu")
ACTS4 = ACTS3 + ("relu6",)


def cases(dev):
    """Yields (name, {array name: tensor}) for every case, in a fixed order."""
    import torch

    from super_gradients_amd import _lib, kernels as K

    def nhwc(t, ld_pix=None, c_off=0):  # a CPU NCHW tensor as an NHWC view on the device, optionally a channel slice of a wider (NaN) buffer
        n, c, h, w = t.shape
        if ld_pix is None:
            return t.permute(0, 2, 3, 1).contiguous().to(dev)
        view = torch.full((n, h, w, ld_pix), float("nan"), device=dev)[..., c_off:c_off + c]
        view.copy_(t.permute(0, 2, 3, 1).to(dev))
        return view

    def out_view(n, h, w, c):
        return torch.full((n, h, w, c + 8), float("nan"), device=dev)[..., 4:4 + c]

    for n, h, w, c in SHAPES:
        g = torch.Generator().manual_seed(3)
        t3, t1, x, r, dy = (torch.randn(n, c, h, w, generator=g) for _ in range(5))
        vec = lambda lo, hi: (torch.rand(c, generator=g) * (hi - lo) + lo).to(dev)  # noqa: E731
        sb = [(vec(0.5, 1.5), vec(-0.3, 0.3)) for _ in range(3)]
        mu = [vec(-0.2, 0.2) for _ in range(3)]
        gam, inv = vec(0.5, 1.5), vec(0.5, 1.5)
        M = n * h * w
        ops = (nhwc(t3, c + 4), nhwc(t1), nhwc(x, c + 12, 8))
        rr, dyd = nhwc(r), nhwc(dy, c + 4)
        tag = f"{n}x{h}x{w}x{c}"
        for act in ACTS3:
            for blocks in (None, 3, M):
                for nb in (1, 2, 3):
                    br = [v for op, (s, b) in zip(ops[:nb], sb) for v in (op, s, b)]
                    for stats in (False, True):
                        for post in (False, True):
                            res = K.tri_affine_act(*br, post_add=rr if post else None, post_scale=0.75 if post else None, act=act, out=out_view(n, h, w, c),
                                                   want_stats=stats, blocks=blocks)
                            y, parts = res if stats else (res, None)
                            yield f"fwd {tag} act={act} blocks={blocks} branches={nb} stats={stats} post={post}", {"y": y, "parts": parts}
                for nb in (1, 2, 3):
                    br = [v for op, (s, b), m in zip(ops[:nb], sb, mu) for v in (op, s, b, m)]
                    try:
                        res = K.tri_affine_act_bwd_reduce(dyd, *br, act=act, out=out_view(n, h, w, c), blocks=blocks)
                    except (TypeError, _lib.SgxError):  # a build whose reduce sweep needs two branches: the case is not in its record
                        if nb > 1:
                            raise
                        continue
                    yield f"bwd_reduce {tag} act={act} blocks={blocks} branches={nb}", {"g": res[0], "p1": res[1], "p2": res[2], "p3": res[3]}
        for act in ACTS4:
            for stats in (False, True):
                res = K.affine_act(ops[0], sb[0][0], sb[0][1], r1=rr, a1=0.5, r2=ops[2], a2=1.25, out=out_view(n, h, w, c), act=act, want_stats=stats)
                y, parts = res if stats else (res, None)
                yield f"affine_act {tag} act={act} stats={stats}", {"y": y, "parts": parts}
            dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
            dx, gg = K.bn_bwd(dyd, ops[0], sb[0][0], sb[0][1], gam, mu[0], inv, dg, db, act=act, dx_out=out_view(n, h, w, c), want_g=True)
            yield f"bn_bwd {tag} act={act}", {"dx": dx, "g": gg, "dgamma": dg, "dbeta": db}
        yield f"channel_stats_partial {tag}", {"parts": K.channel_stats_partial(ops[2])}
        alpha = torch.tensor([0.625], device=dev)
        yield f"axpy {tag}", {"y": K.axpy(ops[0], a=1.5, out=out_view(n, h, w, c))}
        acc = out_view(n, h, w, c)
        acc.copy_(rr)
        yield f"axpy accumulate {tag}", {"y": K.axpy(ops[2], a_dev=alpha, out=acc, accumulate=True)}
        yield f"relu_bwd {tag}", {"g": K.relu_bwd(dyd, ops[1], out=out_view(n, h, w, c))}
        gg, parts = K.relu_bwd_bn_reduce(dyd, ops[1], ops[2], mu[2])
        yield f"relu_bwd_bn_reduce {tag}", {"g": gg, "parts": parts}
        tot = torch.zeros(c, device=dev)
        K.colsum(ops[0], tot, accumulate=False)
        K.colsum(ops[2], tot, accumulate=True)
        yield f"colsum {tag}", {"sum": tot}
        # the QARepVGG backward sweeps: coefficient rows as the forward finalize leaves them (cf: a, c, scale_p, zeros; sv: mean3, invstd3, scale3,
        # shift3, mean_s, invstd_p, scale_p, shift_p), two BatchNorm stand-ins that own the gradient rows
        cf = torch.stack([sb[0][0] * sb[1][0], sb[1][0] * sb[0][1] + sb[1][1], sb[1][0], torch.zeros(c, device=dev)])
        sv = torch.stack([mu[0], inv, sb[0][0], sb[0][1], mu[1], gam, sb[1][0], sb[1][1]])
        for act in ACTS3:
            bns = []
            for _ in range(2):
                wgt, bias = gam.clone(), mu[2].clone()
                wgt.grad, bias.grad = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
                bns.append(types.SimpleNamespace(weight=wgt, bias=bias))
            yv, uv = out_view(n, h, w, c), nhwc(t1)
            yv.copy_(ops[0])
            ds, dyo = K.qarep_bwd(dyd, yv, uv, cf, sv, bns[0], bns[1], act)
            yield f"qarep_bwd {tag} act={act}", {"ds": ds, "dy": dyo, "dgamma3": bns[0].weight.grad, "dgammap": bns[1].weight.grad, "dbetap": bns[1].bias.grad}


def ulps(a, b):
    """Largest distance in units in the last place between two fp32 arrays, and the flat index of the first element that differs."""
    import numpy as np

    def ordered(v):  # the IEEE bit patterns as integers that count representable numbers in order
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(ordered(a) - ordered(b)).ravel()
    return int(d.max()), int(np.flatnonzero(a.view(np.int32).ravel() != b.view(np.int32).ravel())[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=("record", "check"))
    ap.add_argument("file")
    ap.add_argument("--backend", choices=("gpu", "emu"), default="gpu")
    args = ap.parse_args()
    import numpy as np
    import torch

    if args.backend == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import emu_env

        emu_env.activate()
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda:0")
    got = {}
    for name, arrays in cases(dev):
        for k, v in arrays.items():
            if v is not None:
                got[f"{name} / {k}"] = np.ascontiguousarray(v.detach().cpu().numpy())
    if args.mode == "record":
        os.makedirs(os.path.dirname(os.path.abspath(args.file)), exist_ok=True)
        np.savez(args.file, **got)
        print(f"sweep_parity: recorded {len(got)} arrays ({args.backend}) in {args.file}")
        return 0
    want = np.load(args.file)
    bad = 0
    fresh = sorted(set(got) - set(want.files))  # cases the recording build could not run (the one-branch reduce before it existed): nothing to compare
    if fresh:
        print(f"sweep_parity: {len(fresh)} arrays are not in the record and were not compared, e.g. {fresh[0]}")
    for key in sorted(set(want.files) | set(got) - set(fresh)):
        if key not in got:
            bad += 1
            print(f"MISSING {key}: in the record, not produced by this build")
            continue
        a, b = want[key], got[key]
        if a.shape != b.shape:
            bad += 1
            print(f"MISMATCH {key}: shape {a.shape} recorded, {b.shape} now")
        elif not torch.equal(torch.from_numpy(a.view(np.int32)), torch.from_numpy(b.view(np.int32))):
            bad += 1
            worst, first = ulps(a, b)
            print(f"MISMATCH {key}: first differing index {np.unravel_index(first, a.shape)}, largest difference {worst} ulp, "
                  f"{int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} elements")
    print(f"sweep_parity: {len(got) - len(fresh)} arrays checked ({args.backend}), {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
