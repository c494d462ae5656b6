"""The depthwise 3x3 kernels on the distinct depthwise problems of mobilenet_v2 (batch 64, 224 x 224), and the whole model's train step.

    python tools/dwconv_bench.py [--iters 20] [--batch 64] [--size 224] [--steps 10] [--k5]
--k5: the distinct 5x5 problems of mobilenet_v3_large instead - both forms of the 5x5 forward (register window, LDS patch), the data and
weight gradient, the 3x3 kernels' times on the same tensor shape, and mobilenet_v3_large's train step.
Per problem: forward, data gradient and weight gradient, timed with device events after a warm-up, beside their algorithmic bytes (forward
and data gradient read one tensor and write one; the weight gradient reads two) and beside the rate the project's own element sweep
(sgx_affine_act_fwd: one tensor read, one written) reaches at the SAME byte count in the same process - the nearest memory-bound kernel that
is already tuned here.  Then mobilenet_v2's train step (forward, cross-entropy, backward, SGD) in images/s.  Measurement tool: product
library only."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def depthwise_problems(net, size):
    """[(H, W, C, stride, count)] of the model's depthwise layers at a size x size input, in network order, distinct ones once."""
    from super_gradients_amd.training.models.classification_models.mobilenetv2 import InvertedResidual

    h = (size - 1) // 2 + 1  # the stride-2 stem
    seen = {}
    for m in net.modules():
        if isinstance(m, InvertedResidual):
            key = (h, h, m.dw._parts()[0].in_channels, m.stride)
            seen[key] = seen.get(key, 0) + 1
            h = (h - 1) // m.stride + 1
    return [k + (v,) for k, v in seen.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--k5", action="store_true", help="the 5x5 problems of mobilenet_v3_large (both forward forms) and its train step")
    args = ap.parse_args()
    import torch

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaSGD

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

    def sweep_rate(nbytes, c):
        """TB/s of the affine + activation sweep moving `nbytes` in all (half read, half written) over `c` channels"""
        rows = max(nbytes // 2 // 4 // c, 1)
        a = torch.randn(1, 1, rows, c, device=dev)
        b = torch.empty_like(a)
        sc, sh = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
        t = timed(lambda: K.affine_act(a, sc, sh, act="relu6", out=b))
        return 2 * a.numel() * 4 / t / 1e6

    n = args.batch
    name = "mobilenet_v3_large" if args.k5 else "mobilenet_v2"
    net = models.get(name, num_classes=1000)
    if args.k5:
        from super_gradients_amd.training.models.classification_models.mobilenetv3 import InvertedResidual as V3Block

        h, seen = (args.size - 1) // 2 + 1, {}
        for m in net.modules():
            if isinstance(m, V3Block):
                conv = m.dw._parts()[0]
                if conv.kernel_size == 5:
                    seen[(h, h, conv.in_channels, m.stride)] = seen.get((h, h, conv.in_channels, m.stride), 0) + 1
                h = (h - 1) // m.stride + 1
        print(f"mobilenet_v3_large 5x5 depthwise problems, batch {n}, {args.size} x {args.size}; us per call, achieved TB/s from the algorithmic bytes, share of the element "
              "sweep's rate at the same bytes; 3x3: the 3x3 kernels' us on the same tensors (forward / data gradient / weight gradient)")
        print(f"{'H x W x C, stride':<24}{'layers':>7}{'MB in':>8} | {'forward, register':>24} | {'forward, LDS patch':>24} | {'data gradient':>24} | {'weight gradient':>24} | "
              f"{'sweep TB/s':>12} | {'3x3 us':>24}")
        for (h, w, c, s), count in seen.items():
            x = torch.randn(n, h, w, c, device=dev)
            wt, w3 = K.to_dw(torch.randn(c, 1, 5, 5, device=dev)), K.to_dw(torch.randn(c, 1, 3, 3, device=dev))
            y = K.dwconv5x5_fwd(x, wt, stride=s)
            dy, dx, dw, dw3 = torch.randn_like(y), torch.empty_like(x), K.dw_empty(c, dev, 5), K.dw_empty(c, dev)
            dw.zero_()
            dw3.zero_()
            b = x.numel() * 4 + y.numel() * 4
            cols = []
            for form in ("register", "lds"):
                K.set_dwconv5x5_form(form)
                cols.append(timed(lambda: K.dwconv5x5_fwd(x, wt, out=y, stride=s, stat_partials=True)))
            K.set_dwconv5x5_form("register")
            cols.append(timed(lambda: K.dwconv5x5_bwd_data(dy, wt, tuple(x.shape), stride=s, out=dx)))
            cols.append(timed(lambda: K.dwconv5x5_bwd_weight(x, dy, dw, stride=s)))
            t3 = [timed(lambda: K.dwconv3x3_fwd(x, w3, out=y, stride=s, stat_partials=True)), timed(lambda: K.dwconv3x3_bwd_data(dy, w3, tuple(x.shape), stride=s, out=dx)),
                  timed(lambda: K.dwconv3x3_bwd_weight(x, dy, dw3, stride=s))]
            r1 = sweep_rate(b, c)
            print(f"{f'{h} x {w} x {c}, s{s}':<24}{count:>7}{x.numel() * 4 / 1e6:>8.1f} | " + " | ".join(f"{t:>8.1f} {b / t / 1e6:>6.2f} {b / t / 1e6 / r1 * 100:>6.0f} %" for t in cols)
                  + f" | {r1:>12.2f} | " + " / ".join(f"{t:.1f}" for t in t3))
    else:
        print(f"mobilenet_v2 depthwise problems, batch {n}, {args.size} x {args.size}; us per call, achieved TB/s from the algorithmic bytes, share of the element sweep's rate at the same bytes")
        print(f"{'H x W x C, stride':<24}{'layers':>7}{'MB in':>8} | {'forward':>24} | {'data gradient':>24} | {'weight gradient':>24} | {'sweep TB/s':>12}")
        for h, w, c, s, count in depthwise_problems(net, args.size):
            x = torch.randn(n, h, w, c, device=dev)
            wt = K.to_dw(torch.randn(c, 1, 3, 3, device=dev))
            y = K.dwconv3x3_fwd(x, wt, stride=s)
            dy, dx, dw = torch.randn_like(y), torch.empty_like(x), K.dw_empty(c, dev)
            dw.zero_()
            bx, by = x.numel() * 4, y.numel() * 4
            cols = [(timed(lambda: K.dwconv3x3_fwd(x, wt, out=y, stride=s, stat_partials=True)), bx + by),
                    (timed(lambda: K.dwconv3x3_bwd_data(dy, wt, tuple(x.shape), stride=s, out=dx)), bx + by),
                    (timed(lambda: K.dwconv3x3_bwd_weight(x, dy, dw, stride=s)), bx + by)]
            r1 = sweep_rate(bx + by, c)
            print(f"{f'{h} x {w} x {c}, s{s}':<24}{count:>7}{bx / 1e6:>8.1f} | " + " | ".join(f"{t:>8.1f} {b / t / 1e6:>6.2f} {b / t / 1e6 / r1 * 100:>6.0f} %" for t, b in cols)
                  + f" | {r1:>12.2f}")
    # the whole train step
    net.materialize(dev).train()
    opt = ArenaSGD(net, lr=0.01, momentum=0.9, weight_decay=1e-4)
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
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    print(f"{name} train step (forward, cross-entropy, backward, SGD), batch {n}, {args.size} x {args.size}: {dt * 1e3:.2f} ms, {n / dt:.0f} images/s, loss {float(loss):.4f}")


if __name__ == "__main__":
    main()
