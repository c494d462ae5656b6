"""The RepVGG three-branch sweeps against the same work composed from the two-branch entry points, and a whole repvgg_a0 train step.

    python tools/repvgg_bench.py [--iters 50] [--repeats 5] [--batch 64] [--no-step]
Shapes: the identity blocks of RepVggA0 and RepVggB1 at 224 x 224 (stage 1-3; stage 4 is a single stride-2 block).
  forward   fused:    sgx_tri_affine_act_fwd with the statistics rows                              reads t3, t1, x      writes y
            composed: the two-branch sweep (no activation) -> affine_act(x) + residual + ReLU -> channel_stats_partial(y)
                                                                                                    reads t3, t1, x, tmp, y   writes tmp, y
  backward  fused:    sgx_tri_affine_act_bwd_reduce                                                 reads dy, t3, t1, x  writes g
            composed: the two-branch reduce sweep -> sgx_bn_bwd_reduce(g, x)                   reads dy, t3, t1, g, x   writes g
            (the composed backward cannot form the three-term pre-activation: it is timed for its traffic, not compared for its values)
Method: every shape warmed up; the two versions alternate inside each repeat; device events around `iters` launches; median and the
min..max spread over the repeats; bytes = the tensors listed above, 4 B an element.  Measurement tool: product library, GPU only."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/repvgg_bench.py measures on the GPU; none found")
    from super_gradients_amd import kernels as K
    from super_gradients_amd._lib import check, lib
    from super_gradients_amd.kernels import ptr, rows, stats_blocks, stream

    dev = torch.device("cuda:0")
    B = args.batch
    shapes = [("A0 stage1", B, 56, 56, 48), ("A0 stage2", B, 28, 28, 96), ("A0 stage3", B, 14, 14, 192),
              ("B1 stage1", B, 56, 56, 128), ("B1 stage2", B, 28, 28, 256), ("B1 stage3", B, 14, 14, 512)]

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    def versus(a, b):
        for f in (a, b):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(window(a))
            tb.append(window(b))
        return ta, tb

    def fmt(ts, nbytes):
        m = statistics.median(ts)
        return f"{m:8.1f} us ({min(ts):.1f}..{max(ts):.1f})  {nbytes / m / 1e6:5.2f} TB/s"

    print(f"device: {torch.cuda.get_device_name(0)}; iters {args.iters}, repeats {args.repeats}")
    for name, n, h, w, c in shapes:
        t3, t1, x, dy = (torch.randn(n, h, w, c, device=dev) for _ in range(4))
        y, tmp, g = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        sc = [torch.rand(c, device=dev) + 0.5 for _ in range(3)]
        sh = [torch.randn(c, device=dev) * 0.1 for _ in range(3)]
        mu = [torch.randn(c, device=dev) * 0.1 for _ in range(3)]
        nb = x.numel() * 4
        M = n * h * w
        parts2 = torch.empty(2, stats_blocks(M), c, device=dev)

        def fwd_fused():
            K.tri_affine_act(t3, sc[0], sh[0], t1, sc[1], sh[1], x, sc[2], sh[2], act="relu", out=y, want_stats=True)

        def fwd_composed():
            K.tri_affine_act(t3, sc[0], sh[0], t1, sc[1], sh[1], act=None, out=tmp)
            K.affine_act(x, sc[2], sh[2], r1=tmp, act="relu", out=y)
            K.channel_stats_partial(y)

        def bwd_fused():
            K.tri_affine_act_bwd_reduce(dy, t3, sc[0], sh[0], mu[0], t1, sc[1], sh[1], mu[1], x, sc[2], sh[2], mu[2], act="relu", out=g)

        def bwd_composed():
            K.tri_affine_act_bwd_reduce(dy, t3, sc[0], sh[0], mu[0], t1, sc[1], sh[1], mu[1], act="relu", out=g)
            check(lib().sgx_bn_bwd_reduce(ptr(g), rows(g)[1], ptr(x), rows(x)[1], ptr(sc[2]), ptr(sh[2]), ptr(mu[2]), M, c, K.ACT[None], ptr(parts2),
                                          stream()), "sgx_bn_bwd_reduce")

        # the fused forward against the composition, on the same inputs (section 6 of the measuring guide: faster and different is not faster)
        fwd_fused()
        y_f = y.clone()
        fwd_composed()
        err = float((y_f - y).abs().max() / y.abs().max())
        ff, fc = versus(fwd_fused, fwd_composed)
        bf, bc = versus(bwd_fused, bwd_composed)
        print(f"{name:<10} {str((n, h, w, c)):<20} {nb / 1e6:7.1f} MB/tensor  fused-vs-composed y: {err:.1e}")
        print(f"    forward   fused {fmt(ff, 4 * nb)}   composed {fmt(fc, 7 * nb)}   ratio {statistics.median(fc) / statistics.median(ff):.2f}")
        print(f"    backward  fused {fmt(bf, 5 * nb)}   composed {fmt(bc, 6 * nb)}   ratio {statistics.median(bc) / statistics.median(bf):.2f}")
    if args.no_step:
        return
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaSGD

    torch.manual_seed(0)
    net = models.get("repvgg_a0", num_classes=1000)
    net.materialize(dev).train()
    opt = ArenaSGD(net, lr=0.01, momentum=0.9, weight_decay=1e-4, zero_weight_decay_on_bias_and_bn=True)
    loss_fn = CrossEntropyLoss()
    xb = torch.randn(B, 3, 224, 224, device=dev)
    yb = torch.randint(0, 1000, (B,), device=dev)

    def step():
        loss = loss_fn(net(xb), yb)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / args.steps)
    m = statistics.median(ts)
    print(f"repvgg_a0 train step (forward, CE, backward, SGD), batch {B} x 3 x 224 x 224: {m:.2f} ms ({min(ts):.2f}..{max(ts):.2f}) = {B / m * 1e3:.0f} images/s; "
          f"loss {float(loss.detach()):.4f}")


if __name__ == "__main__":
    main()
