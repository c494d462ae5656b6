"""The grouped 3x3 kernels (csrc/gconv.h) on the distinct grouped problems of regnetY800, regnetY200 and resnext50 (batch 64, 224 x 224), and
the whole train steps of regnetY800 and resnext50.

    python tools/gconv_bench.py [--iters 20] [--batch 64] [--size 224] [--steps 10] [--repeats 3] [--models regnetY800,regnetY200,resnext50]
Per problem and pass (forward with statistics rows, data gradient, weight gradient), timed with device events after a warm-up: us per call
(the median of --repeats runs of the whole table and their spread, (max - min) / median), TFLOP/s from 2 * 9 * cg * C * output pixels, TB/s from the
algorithmic bytes (one tensor read and one written; the weight gradient reads two) and the share of the derived roofline - the time the
bytes take at 6.3 TB/s for cg <= 8, the time the FLOP take at 157 TFLOP/s for cg >= 32, the larger of the two at cg = 16.
Beside them, in the same process, the two ways to run the problem on the dense kernels (baselines, not product paths):
    dense: ONE sgx_conv2d_* launch on the filter expanded to block-diagonal form (G x the FLOP);
    slices: G dense launches over channel slices of the tensors (strided views) and of the filter.
Then regnetY800's (RMSpropTF) and resnext50's (SGD) train step (forward, cross-entropy, backward, optimizer) in images/s.  Measurement
tool: product library only."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS, MATRIX_TFS = 6.3, 157.0


def grouped_problems(net, size):
    """[(H, W, C, groups, stride, count)] of the model's grouped layers at a size x size input, in network order, distinct ones once: the map a
    layer sees follows from the strides of the layers before it (RegNet: the stride-2 stem; ResNeXt: the stride-2 stem and the max-pool)."""
    from super_gradients_amd.modules.layers import GroupedConvLayer
    from super_gradients_amd.training.models.classification_models.resnext import ResNeXt

    h = (size - 1) // 2 + 1
    if isinstance(net, ResNeXt):
        h = (h - 1) // 2 + 1
    seen = {}
    for m in net.modules():
        if isinstance(m, GroupedConvLayer):
            key = (h, h, m.in_channels, m.groups, m.stride)
            seen[key] = seen.get(key, 0) + 1
            h = (h - 1) // m.stride + 1
    return [k + (v,) for k, v in seen.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", default="regnetY800,regnetY200,resnext50")
    args = ap.parse_args()
    import torch

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaRMSpropTF, ArenaSGD

    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters  # us

    n = args.batch
    problems = {}
    for name in args.models.split(","):
        for h, w, c, g, s, count in grouped_problems(models.get(name, num_classes=1000), args.size):
            problems.setdefault((h, w, c, g, s), []).append(f"{name} x{count}")
    results = {}  # (problem, pass, variant) -> [us per repeat]
    for rep in range(args.repeats):
        for (h, w, c, g, s) in problems:
            cg = c // g
            x = torch.randn(n, h, w, c, device=dev)
            wt = torch.randn(c, cg, 3, 3, device=dev) / (3.0 * cg ** 0.5)
            wk = K.to_ohwi(wt)
            y = K.gconv3x3_fwd(x, wk, g, stride=s)
            dy, dx, dw = torch.randn_like(y), torch.empty_like(x), K.ohwi_empty(c, cg, 3, 3, dev)
            dw.zero_()
            wbd = torch.zeros(c, c, 3, 3, device=dev)
            for i in range(g):
                wbd[i * cg:(i + 1) * cg, i * cg:(i + 1) * cg] = wt[i * cg:(i + 1) * cg]
            wbd = K.to_ohwi(wbd)
            dwbd = K.ohwi_empty(c, c, 3, 3, dev)
            dwbd.zero_()
            sl = [slice(i * cg, (i + 1) * cg) for i in range(g)]
            ws = [K.to_ohwi(wt[q]) for q in sl]
            dws = [K.ohwi_empty(cg, cg, 3, 3, dev) for _ in sl]
            for t in dws:
                t.zero_()
            shape = tuple(x.shape)
            sshape = shape[:3] + (cg,)

            def slices_fwd():
                for q, wq in zip(sl, ws):
                    K.conv2d_fwd(x[..., q], wq, out=y[..., q], stride=s, pad=1, stat_partials=True)

            def slices_dgrad():
                for q, wq in zip(sl, ws):
                    K.conv2d_bwd_data(dy[..., q], wq, sshape, stride=s, pad=1, out=dx[..., q])

            def slices_wgrad():
                for q, dq in zip(sl, dws):
                    K.conv2d_bwd_weight(x[..., q], dy[..., q], dq, stride=s, pad=1)

            runs = {("fwd", "gconv"): lambda: K.gconv3x3_fwd(x, wk, g, out=y, stride=s, stat_partials=True),
                    ("fwd", "dense"): lambda: K.conv2d_fwd(x, wbd, out=y, stride=s, pad=1, stat_partials=True),
                    ("fwd", "slices"): slices_fwd,
                    ("dgrad", "gconv"): lambda: K.gconv3x3_bwd_data(dy, wk, g, shape, stride=s, out=dx),
                    ("dgrad", "dense"): lambda: K.conv2d_bwd_data(dy, wbd, shape, stride=s, pad=1, out=dx),
                    ("dgrad", "slices"): slices_dgrad,
                    ("wgrad", "gconv"): lambda: K.gconv3x3_bwd_weight(x, dy, dw, g, stride=s),
                    ("wgrad", "dense"): lambda: K.conv2d_bwd_weight(x, dy, dwbd, stride=s, pad=1),
                    ("wgrad", "slices"): slices_wgrad}
            for (p, v), fn in runs.items():
                try:
                    t = timed(fn)
                except Exception as e:  # a baseline the dense kernels refuse (the product path raises)
                    if v == "gconv":
                        raise
                    if rep == 0:
                        print(f"# {h} x {w} x {c}, G {g}, s{s}: {p} / {v} not available: {str(e)[:120]}")
                    t = float("nan")
                results.setdefault(((h, w, c, g, s), p, v), []).append(t)
            del x, y, dy, dx, wbd, dwbd

    def med(ts):
        return statistics.median(ts)

    print(f"grouped 3x3 problems, batch {n}, {args.size} x {args.size}; {args.repeats} runs of the table: median us per call (spread = (max - min) / median), "
          f"TFLOP/s, TB/s, share of the derived roofline; dense / slices: the two baselines' us; x: the faster baseline over gconv")
    print(f"{'H x W x C, cg x G, stride':<30}{'pass':>6} | {'gconv us':>9} {'spread':>7} {'TF/s':>7} {'TB/s':>6} {'roof':>6} | {'dense us':>9} {'spread':>7} | {'slices us':>9} {'spread':>7} | {'x':>6}  layers")
    for (h, w, c, g, s), who in problems.items():
        cg = c // g
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        flops = 2.0 * 9 * cg * c * n * ho * wo
        bx, by = n * h * w * c * 4.0, n * ho * wo * c * 4.0
        for p in ("fwd", "dgrad", "wgrad"):
            ts = {v: results[((h, w, c, g, s), p, v)] for v in ("gconv", "dense", "slices")}
            t = med(ts["gconv"])
            t_mem, t_mat = (bx + by) / HBM_TBS / 1e6, flops / MATRIX_TFS / 1e6  # us
            roof = t_mem if cg <= 8 else (t_mat if cg >= 32 else max(t_mem, t_mat))
            best = min(med(ts["dense"]), med(ts["slices"]))
            sp = {v: (max(ts[v]) - min(ts[v])) / med(ts[v]) * 100 for v in ts}
            print(f"{f'{h} x {w} x {c}, {cg} x {g}, s{s}':<30}{p:>6} | {t:>9.1f} {sp['gconv']:>6.1f}% {flops / t / 1e6:>7.1f} {(bx + by) / t / 1e6:>6.2f} {roof / t * 100:>5.0f}% | "
                  f"{med(ts['dense']):>9.1f} {sp['dense']:>6.1f}% | {med(ts['slices']):>9.1f} {sp['slices']:>6.1f}% | {best / t:>6.2f}  {', '.join(who)}")
    # the whole train steps
    for name, make_opt in (("regnetY800", lambda net: ArenaRMSpropTF(net, lr=0.016, alpha=0.9, momentum=0.9, eps=0.001, weight_decay=1e-5)),
                           ("resnext50", lambda net: ArenaSGD(net, lr=0.01, momentum=0.9, weight_decay=1e-4))):
        if not args.steps:
            break
        net = models.get(name, num_classes=1000)
        net.materialize(dev).train()
        opt = make_opt(net)
        loss_fn = CrossEntropyLoss()
        xb, yb = torch.randn(n, 3, args.size, args.size, device=dev), torch.randint(0, 1000, (n,), device=dev)

        def step():
            loss = loss_fn(net(xb), yb)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.steps)
        dt = med(times)
        print(f"{name} train step (forward, cross-entropy, backward, {type(opt).__name__[5:]}), batch {n}, {args.size} x {args.size}: {dt * 1e3:.2f} ms "
              f"(spread {(max(times) - min(times)) / dt * 100:.1f}%), {n / dt:.0f} images/s, loss {float(loss):.4f}")
        del net, opt


if __name__ == "__main__":
    main()
