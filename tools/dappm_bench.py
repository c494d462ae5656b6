"""The DAPPM kernels (csrc/dappm.h) and the whole module at DDRNet's 1/64 map of a 1024 x 2048 image: N = 16, 16 x 32 pixels,
in 1024 / branch 128 / out 256 (DDRNet23) and in 512 / 64 / 128 (DDRNet23-slim) - the two pyramid launches alone, and the module's training
forward and forward + backward next to the same module composed from plain torch operations on the device (avg_pool2d, batch_norm, relu,
conv2d, interpolate, cat: what a user had before these kernels).

    python tools/dappm_bench.py [--iters 50] [--repeats 5] [--batch 16]
    rocprofv3 --kernel-trace --stats ... -- python tools/dappm_bench.py --pyramid-only 200      (kernel times, in a run of their own)
Every figure this tool prints is a CALL time: device events around --iters calls of the Python wrapper after a warm-up, so the wrapper's
allocations and the launch are inside it; the calls are interleaved inside every repeat, us per call is the median of --repeats runs with the
spread (max - min) / median.  It is no kernel time: for the two pyramid launches the tool prints their ALGORITHMIC bytes (forward: one read of
x; backward: one write of dx and one read of each addend) and the time those bytes take at the HBM's 8 TB/s, to set beside the kernel times
of a trace (--pyramid-only runs nothing but the two launches, for that trace).  Measurement tool: product library only, needs the GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0
KERNELS, STRIDES = [1, 5, 9, 17, 0], [1, 2, 4, 8, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pyramid-only", type=int, default=0, metavar="CALLS", help="run only the two pyramid launches, CALLS times each (for a kernel trace)")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from torch import nn

    from super_gradients_amd import kernels as K
    from super_gradients_amd.modules.engine import SgxNetwork
    from super_gradients_amd.training.models.segmentation_models import DAPPM

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

    class TorchDAPPM(nn.Module):  # the module as a chain of ATen operations, NCHW
        def __init__(self, cin, cb, cout):
            super().__init__()
            bnconv = lambda a, b, k: nn.Sequential(nn.BatchNorm2d(a), nn.ReLU(), nn.Conv2d(a, b, k, padding=k // 2, bias=False))  # noqa: E731
            self.down = nn.ModuleList([bnconv(cin, cb, 1) for _ in STRIDES])
            self.process = nn.ModuleList([bnconv(cb, cb, 3) for _ in STRIDES[1:]])
            self.compression, self.shortcut = bnconv(cb * len(STRIDES), cout, 1), bnconv(cin, cout, 1)

        def forward(self, x):
            outs = [self.down[0](x)]
            for i, (k, s) in enumerate(zip(KERNELS[1:], STRIDES[1:]), 1):
                p = F.avg_pool2d(x, k, s, s) if s else F.adaptive_avg_pool2d(x, 1)
                up = F.interpolate(self.down[i](p), size=x.shape[2:], mode="bilinear")
                outs.append(self.process[i - 1](up + outs[-1]))
            return self.compression(torch.cat(outs, 1)) + self.shortcut(x)

    class Net(SgxNetwork):
        def __init__(self, blk):
            super().__init__()
            self.add_module("0", blk)

    n, h, w = args.batch, 16, 32
    levels = [(k, s) for k, s in zip(KERNELS, STRIDES) if s > 1]
    for cin, cb, cout in ((1024, 128, 256), (512, 64, 128)):
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(n, h, w, cin, device=dev, generator=g)
        dy = torch.randn(n, h, w, cout, device=dev, generator=g)
        pooled, _ = K.dappm_pool_fwd(x, levels, True)
        adds = [torch.randn_like(x), torch.randn_like(x)]
        dxbuf = torch.empty_like(x)
        xb = 4.0 * x.numel()
        print(f"N = {n}, {h} x {w}, in {cin} / branch {cb} / out {cout}: dappm_pool_fwd reads x once = {xb / 1e6:.1f} MB ({xb / HBM_TBS / 1e6:.1f} us at "
              f"{HBM_TBS:.0f} TB/s), dappm_pool_bwd with two addends moves {3 * xb / 1e6:.1f} MB ({3 * xb / HBM_TBS / 1e6:.1f} us)")
        if args.pyramid_only:
            for _ in range(args.pyramid_only):
                K.dappm_pool_fwd(x, levels, True)
                K.dappm_pool_bwd(pooled[:3], levels, tuple(x.shape), d_global=pooled[3], addends=adds, out=dxbuf)
            torch.cuda.synchronize()
            continue
        blk = DAPPM(cin, cb, cout, KERNELS, STRIDES)
        net = Net(blk).materialize(dev).train()
        ref = TorchDAPPM(cin, cb, cout).to(dev).train()
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
        dyt = dy.permute(0, 3, 1, 2).contiguous()

        def sgx_step():
            blk.fwd(x)
            blk.bwd(dy)
            net.join_side()  # (the weight gradients run on the side stream)

        def torch_step():
            xt.grad = None
            ref(xt).backward(dyt)

        calls = {"dappm_pool_fwd call": lambda: K.dappm_pool_fwd(x, levels, True),
                 "dappm_pool_bwd call": lambda: K.dappm_pool_bwd(pooled[:3], levels, tuple(x.shape), d_global=pooled[3], addends=adds, out=dxbuf),
                 "module forward": lambda: blk.fwd(x),
                 "module forward in torch": lambda: ref(xt),
                 "module forward + backward": sgx_step,
                 "module forward + backward in torch": torch_step}
        res = {}
        for _ in range(args.repeats):
            for name, fn in calls.items():
                res.setdefault(name, []).append(timed(fn))
        print(f"call times (wrapper allocations and launches included; no kernel times), {args.iters} iterations, median of {args.repeats} repeats")
        med = {name: statistics.median(us) for name, us in res.items()}
        for name, us in res.items():
            print(f"{name:36s} {med[name]:9.1f} us (spread {(max(us) - min(us)) / med[name]:5.1%})")
        for name in ("module forward", "module forward + backward"):
            print(f"{name}: {med[name + ' in torch'] / med[name]:.2f} x the speed of the torch composition")

if __name__ == "__main__":
    main()
