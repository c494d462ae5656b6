"""The BatchNorm -> SiLU -> SE gate sweeps (csrc/se.hip: sgx_bn_act_gate_*) on the distinct depthwise + SE problems of efficientnet_b0
(batch 64, 224 x 224), against the sequence the entry points that existed before them force, and the whole efficientnet_b0 train step.

    python tools/mbconv_bench.py [--iters 20] [--batch 64] [--size 224] [--steps 10] [--repeats 3] [--model efficientnet_b0]
Per problem (the depthwise layer's output map t [N, H, W, C], C the expanded width) and direction, timed with device events after a
warm-up: us per call sequence (the median of --repeats runs of the whole table and their spread, (max - min) / median) and TB/s from the
algorithmic bytes.  The SE layer's two small convolutions on [N,1,1,C] are the same on both sides and are left out.
    fused forward    bn_act_gate_mean(t) + bn_act_gate_fwd(t -> y)                                   2 reads, 1 write of the map
    baseline forward affine_act(t -> a, SiLU) + image_colsum(a) + channel_gate(a -> y)               3 reads, 2 writes
    fused backward   bn_act_gate_bwd_gate(dy, t) + bn_act_gate_bwd_data(dy, t -> dz, reduce rows)    4 reads, 1 write
    baseline backward image_colsum(dy, a) + channel_gate(dy -> da) + bn_bwd_reduce(da, t)            5 reads, 1 write (and a kept alive)
From bytes alone the forward should approach 3/5 of the baseline's time and the backward 5/6.  Then the model's train step (forward,
label-smoothed cross-entropy, backward, RMSpropTF) in images/s.  Measurement tool: product library only."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def se_problems(net, size):
    """[(H, W, C, count, blocks)] of the model's depthwise outputs that feed an SE layer at a size x size input, distinct ones once"""
    h = (size - 1) // 2 + 1  # the stride-2 stem
    seen = {}
    for i, blk in enumerate(net._blocks):
        h = (h - 1) // blk._depthwise_conv.stride + 1
        if blk._se is not None:
            seen.setdefault((h, h, blk._depthwise_conv.out_channels), []).append(i)
    return [k + (len(v), v) for k, v in seen.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="efficientnet_b0")
    args = ap.parse_args()
    import torch

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaRMSpropTF

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
    problems = se_problems(models.get(args.model, arch_params=dict(image_size=args.size), num_classes=1000), args.size)
    results = {}
    L, SILU = K.lib(), K.ACT["silu"]
    for rep in range(args.repeats):
        for (h, w, c, _, _) in problems:
            m = n * h * w
            t, dy = torch.randn(n, h, w, c, device=dev), torch.randn(n, h, w, c, device=dev)
            sc, sh, mean = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev), torch.randn(c, device=dev) * 0.1
            pre, dmean = torch.randn(n, c, device=dev), torch.randn(n, c, device=dev)
            a, y, dz, da = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
            parts = torch.empty(2, K.stats_blocks(m), c, device=dev)

            def fused_fwd():
                K.bn_act_gate_mean(t, sc, sh, act="silu")
                K.bn_act_gate_fwd(t, sc, sh, pre, "sigmoid", act="silu", out=y)

            def base_fwd():
                K.affine_act(t, sc, sh, act="silu", out=a)
                K.image_colsum(a, scale=1.0 / (h * w))
                K.channel_gate(a, pre, "sigmoid", out=y)

            def fused_bwd():
                K.bn_act_gate_bwd_gate(dy, t, sc, sh, pre, "sigmoid", act="silu")
                K.bn_act_gate_bwd_data(dy, t, sc, sh, pre, "sigmoid", act="silu", dmean=dmean, save_mean=mean, out=dz, want_parts=True)

            def base_bwd():
                K.image_colsum(dy, v=a, pre=pre, gate="sigmoid")
                K.channel_gate(dy, pre, "sigmoid", bias=dmean, bias_scale=1.0 / (h * w), out=da)
                K.check(L.sgx_bn_bwd_reduce(K.ptr(da), c, K.ptr(t), c, K.ptr(sc), K.ptr(sh), K.ptr(mean), m, c, SILU, K.ptr(parts), K.stream()), "sgx_bn_bwd_reduce")

            base_fwd()  # (a for the baseline backward)
            for key, fn in (("fwd", "fused"), fused_fwd), (("fwd", "base"), base_fwd), (("bwd", "fused"), fused_bwd), (("bwd", "base"), base_bwd):
                results.setdefault(((h, w, c),) + key, []).append(timed(fn))
            del t, dy, a, y, dz, da

    med = statistics.median
    print(f"{args.model} depthwise + SE problems, batch {n}, {args.size} x {args.size}; {args.repeats} runs of the table: median us per sequence "
          f"(spread = (max - min) / median), TB/s from the algorithmic bytes; ratio = fused / baseline (bytes alone: forward 0.60, backward 0.83)")
    print(f"{'H x W x C':<18}{'pass':>5} | {'fused us':>9} {'spread':>7} {'TB/s':>6} | {'base us':>9} {'spread':>7} {'TB/s':>6} | {'ratio':>6}  blocks")
    for (h, w, c, count, blocks) in problems:
        b = n * h * w * c * 4.0
        for p, pf, pb in (("fwd", 3, 5), ("bwd", 5, 6)):
            tf, tb = results[((h, w, c), p, "fused")], results[((h, w, c), p, "base")]
            sf, sb = (max(tf) - min(tf)) / med(tf) * 100, (max(tb) - min(tb)) / med(tb) * 100
            print(f"{f'{h} x {w} x {c}':<18}{p:>5} | {med(tf):>9.1f} {sf:>6.1f}% {pf * b / med(tf) / 1e6:>6.2f} | {med(tb):>9.1f} {sb:>6.1f}% {pb * b / med(tb) / 1e6:>6.2f} | "
                  f"{med(tf) / med(tb):>6.2f}  {blocks}")
    if not args.steps:
        return
    net = models.get(args.model, arch_params=dict(image_size=args.size), num_classes=1000)
    net.materialize(dev).train()
    opt = ArenaRMSpropTF(net, lr=0.016, alpha=0.9, momentum=0.9, eps=0.001, weight_decay=1e-5)
    loss_fn = CrossEntropyLoss(smooth_eps=0.1)
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
    print(f"{args.model} train step (forward, label-smoothed cross-entropy, backward, RMSpropTF; drop-connect {net.drop_connect_rate}, dropout {net._dropout.p}), "
          f"batch {n}, {args.size} x {args.size}: {dt * 1e3:.2f} ms (spread {(max(times) - min(times)) / dt * 100:.1f}%), {n / dt:.0f} images/s, loss {float(loss.detach()):.4f}")


if __name__ == "__main__":
    main()
