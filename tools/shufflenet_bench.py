"""The ShuffleNetV2 kernels (csrc/shuffle.h) on the stage shapes of shufflenet_v2_x1_5 and shufflenet_v2_x0_5 (batch 64, 224 x 224), and the
train step of shufflenet_v2_x1_5.

    python tools/shufflenet_bench.py [--iters 20] [--batch 64] [--size 224] [--steps 10]
Per stage map, the three merge kernels in the one-sided form (left side a copy: the stride-1 block) and the two-sided form (both sides
affine + ReLU: the stride-2 block), timed with device events after a warm-up, beside their algorithmic bytes (floats per pixel, h the half
width) and beside the rate the project's own element sweep (sgx_affine_act_fwd: one tensor read, one written) reaches at the SAME byte count
in the same process:
  forward   reads 2h, writes 2h
  reduce    reads dy (2h) and the saved conv output of every affine side: 3h one-sided, 4h two-sided
  apply     reads dy (2h) and x of every affine side, writes 2h: 5h one-sided, 6h two-sided
Then shufflenet_v2_x1_5's train step (forward, cross-entropy, backward, SGD) in images/s - an absolute figure: no earlier build has the model.
Measurement tool: product library only."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
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
        t = timed(lambda: K.affine_act(a, sc, sh, act="relu", out=b))
        return 2 * a.numel() * 4 / t / 1e6

    def cell(t, b, c):
        r1 = sweep_rate(b, c)
        return f"{t:>7.1f} {b / t / 1e6:>5.2f} {b / t / 1e6 / r1 * 100:>5.0f} %"

    n = args.batch
    s = ((args.size - 1) // 2 + 1 - 1) // 2 + 1  # the stride-2 stem and the stride-2 max-pool
    print(f"ShuffleNetV2 merge kernels, batch {n}, {args.size} x {args.size}, {args.iters} timed calls each after 3 warm-up calls; per cell: us per call, "
          "achieved TB/s from the algorithmic bytes, share of the element sweep's rate at the same bytes")
    print(f"{'model / H x W x 2h':<24}{'form':<10} | {'forward':>22} | {'backward reduce':>22} | {'backward apply':>22}")
    for name, widths in (("x1_5", (176, 352, 704)), ("x0_5", (48, 96, 192))):
        hw = s
        for c2 in widths:
            hw = (hw - 1) // 2 + 1  # each stage opens with a stride-2 block
            h = c2 // 2
            pix = n * hw * hw
            xin = torch.randn(n, hw, hw, c2, device=dev)  # the stride-1 block's input: the copy side is its left channel slice
            tl, tr = torch.randn(n, hw, hw, h, device=dev), torch.randn(n, hw, hw, h, device=dev)
            y, dy, dx = torch.empty(n, hw, hw, c2, device=dev), torch.randn(n, hw, hw, c2, device=dev), torch.empty(n, hw, hw, c2, device=dev)
            dtl, dtr = torch.empty_like(tl), torch.empty_like(tr)
            sc, sh, mean = torch.rand(h, device=dev) + 0.5, torch.randn(h, device=dev), torch.randn(h, device=dev)
            coef = torch.rand(5, h, device=dev) * 1e-3
            red, app_l, app_r = (sc, sh, mean, "relu"), (tl, sc, sh, coef, "relu", dtl), (tr, sc, sh, coef, "relu", dtr)
            one = [(timed(lambda: K.shuffle_merge(xin[..., :h], tr, rscale=sc, rshift=sh, ract="relu", out=y)), 4 * h),
                   (timed(lambda: K.shuffle_merge_bwd_reduce(dy, None, (tr,) + red)), 3 * h),
                   (timed(lambda: K.shuffle_merge_bwd_apply(dy, dx[..., :h], app_r)), 5 * h)]
            two = [(timed(lambda: K.shuffle_merge(tl, tr, lscale=sc, lshift=sh, lact="relu", rscale=sc, rshift=sh, ract="relu", out=y)), 4 * h),
                   (timed(lambda: K.shuffle_merge_bwd_reduce(dy, (tl,) + red, (tr,) + red)), 4 * h),
                   (timed(lambda: K.shuffle_merge_bwd_apply(dy, app_l, app_r)), 6 * h)]
            for form, cols in (("one-sided", one), ("two-sided", two)):
                print(f"{f'{name} {hw} x {hw} x {c2}':<24}{form:<10} | " + " | ".join(cell(t, f * pix * 4, h) for t, f in cols))
    # the whole train step
    net = models.get("shufflenet_v2_x1_5", num_classes=1000)
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
    print(f"\nshufflenet_v2_x1_5 train step (forward, cross-entropy, backward, SGD), batch {n}, {args.size} x {args.size}, {args.steps} timed steps after 3: "
          f"{dt * 1e3:.2f} ms, {n / dt:.0f} images/s, loss {float(loss.detach()):.4f}; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


if __name__ == "__main__":
    main()
