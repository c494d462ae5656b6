"""Times the pool-projection kernels (csrc/inception.h) at GoogLeNet's nine branch-4 shapes (batch 64, 224 x 224 input) against the composition
they replace, in the same process: sgx_maxpool_fwd + sgx_conv2d_fwd, sgx_conv2d_bwd_data + sgx_maxpool_bwd, sgx_conv2d_bwd_weight on a stored
pooled map.  Then one googlenet_v1 train step.  Median of `--iters` launches after `--warmup`, HIP events around each launch sequence.

    python tools/inception_bench.py [--batch 64] [--iters 30] [--warmup 5] [--no-step]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from super_gradients_amd import kernels as K  # noqa: E402

# (name, H = W, Ci, Co) of Inception.branch4 in googlenet_v1
SHAPES = [("3a", 28, 192, 32), ("3b", 28, 256, 64), ("4a", 14, 480, 64), ("4b", 14, 512, 64), ("4c", 14, 512, 64), ("4d", 14, 512, 64),
          ("4e", 14, 528, 128), ("5a", 7, 832, 128), ("5b", 7, 832, 128)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(f"pool-projection kernels, batch {a.batch}, median of {a.iters} launches (us): fused | composition")
    print(f"{'block':>5} {'map':>5} {'Ci':>4} {'Co':>4} | {'fwd':>8} {'pool+conv':>9} | {'dgrad':>8} {'conv+pool':>9} | {'wgrad':>8} {'stored':>8}")
    tot = [0.0] * 6
    for name, hw, ci, co in SHAPES:
        x = torch.relu(torch.randn(a.batch, hw, hw, ci, generator=g)).to(dev)
        w = K.to_ohwi((torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5).to(dev))
        dy = torch.randn(a.batch, hw, hw, co, generator=g).to(dev)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.zeros_like(w)
        pooled, am = K.maxpool_fwd(x, 3, 1, 1)
        dpool = torch.empty_like(x)

        def comp_fwd():
            K.maxpool_fwd(x, 3, 1, 1, out=pooled)
            K.conv2d_fwd(pooled, w, out=y)

        def comp_dgrad():
            K.conv2d_bwd_data(dy, w, tuple(x.shape), out=dpool)
            K.maxpool_bwd(dpool, am, tuple(x.shape), 3, 1, 1, out=dx)

        t = [timed(lambda: K.pool3_conv1x1_fwd(x, w, out=y), a.iters, a.warmup), timed(comp_fwd, a.iters, a.warmup),
             timed(lambda: K.pool3_conv1x1_bwd_data(dy, w, x, out=dx), a.iters, a.warmup), timed(comp_dgrad, a.iters, a.warmup),
             timed(lambda: K.pool3_conv1x1_bwd_weight(x, dy, dw), a.iters, a.warmup), timed(lambda: K.conv2d_bwd_weight(pooled, dy, dw), a.iters, a.warmup)]
        tot = [s + v for s, v in zip(tot, t)]
        print(f"{name:>5} {hw:>5} {ci:>4} {co:>4} | {t[0]:8.1f} {t[1]:9.1f} | {t[2]:8.1f} {t[3]:9.1f} | {t[4]:8.1f} {t[5]:8.1f}")
    print(f"{'sum':>5} {'':>5} {'':>4} {'':>4} | {tot[0]:8.1f} {tot[1]:9.1f} | {tot[2]:8.1f} {tot[3]:9.1f} | {tot[4]:8.1f} {tot[5]:8.1f}")
    if a.no_step:
        return
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss
    from super_gradients_amd.training.utils.optimizers import ArenaSGD

    torch.manual_seed(0)
    net = models.get("googlenet_v1", num_classes=1000)
    net.materialize(dev).train()
    opt = ArenaSGD(net, lr=0.01, momentum=0.9, weight_decay=1e-4)
    xb, yb = torch.randn(a.batch, 3, 224, 224, generator=g).to(dev), torch.randint(0, 1000, (a.batch,), generator=g).to(dev)
    loss_fn = CrossEntropyLoss()
    last = [0.0]

    def step():
        loss = loss_fn(net(xb), yb)
        loss.backward()
        opt.step()
        opt.zero_grad()
        last[0] = loss

    torch.cuda.reset_peak_memory_stats()
    us = timed(step, 10, 3)
    print(f"googlenet_v1 train step (forward, cross-entropy, backward, SGD), batch {a.batch}, 224 x 224, 10 timed steps after 3: {us / 1e3:.2f} ms, "
          f"{a.batch / us * 1e6:.0f} images/s, loss {float(last[0].detach()):.4f}; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


if __name__ == "__main__":
    main()
