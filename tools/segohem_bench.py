"""The hard-pixel mining loss (csrc/seg_ohem.h) at the Cityscapes recipe's logit map, 16 x 19 x 1024 x 2048, in both of its
branches, next to seg_ce on the same inputs.

    python tools/segohem_bench.py [--iters 20] [--repeats 3] [--batch 16]
`bar`: threshold 0.7, most pixels lie above it (DDRNetLoss's setting: the mean of the losses above the bar, no selection by rank).
`top-k`: threshold 1e-4, the rank decides: all three radix levels, the sum pass, and a gradient pass most of whose workgroups hold a selected
pixel (mining_percent 0.1 of uniformly random pixels).
Timed with device events after a warm-up, the calls interleaved inside every repeat; us per call is the median of --repeats runs with the
spread (max - min) / median.  Every figure is the whole call (ten launches for seg_ohem_ce, two for seg_ce).  Measurement tool: product library
only, needs the GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from super_gradients_amd import kernels as K

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

    n, c, h, w, ignore = args.batch, 19, 1024, 2048, 19
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(n, c, h, w, device=dev, generator=g)
    labels = torch.randint(0, c + 1, (n, h, w), device=dev, generator=g)  # (the value c is the ignored label)
    calls = {"seg_ce": lambda: K.seg_ce(logits, labels, None, ignore, "mean"),
             "seg_ohem_ce bar": lambda: K.seg_ohem_ce(logits, labels, 0.7, 0.1, ignore, False),
             "seg_ohem_ce top-k": lambda: K.seg_ohem_ce(logits, labels, 1e-4, 0.1, ignore, True)}
    res = {}
    for _ in range(args.repeats):
        for name, fn in calls.items():
            res.setdefault(name, []).append(timed(fn))
    print(f"{n} x {c} x {h} x {w}, {args.iters} iterations, median of {args.repeats} repeats")
    for name, us in res.items():
        print(f"{name:18s} {statistics.median(us):9.1f} us (spread {(max(us) - min(us)) / statistics.median(us):5.1%})")


if __name__ == "__main__":
    main()
