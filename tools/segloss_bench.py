"""The segmentation loss / metric kernels (csrc/segloss.h) at the shapes they are for: the Cityscapes recipe's logit map 16 x 19 x 1024 x 2048
(seg_ce's register-resident form) and an ADE20K-sized one, 16 x 150 x 512 x 512 (the streaming form).

    python tools/segloss_bench.py [--iters 20] [--repeats 3] [--batch 16]
Timed with device events after a warm-up, the kernels interleaved inside every repeat; us per call is the median of --repeats runs with the
spread (max - min) / median.  TB/s is the ALGORITHMIC byte count over that time - seg_ce: the map once, the labels once, the gradient once
(the streaming form really reads the map twice: its figure is against what the algorithm needs, not what it moves); seg_confusion: the map
and the labels once - against 6.3 TB/s.  seg_ce's time includes its one-workgroup fold of the partial sums.  Measurement tool: product
library only, needs the GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


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

    print(f"{args.iters} iterations, median of {args.repeats} repeats")
    for n, c, h, w, ignore in ((args.batch, 19, 1024, 2048, 19), (args.batch, 150, 512, 512, 255)):
        g = torch.Generator(device=dev).manual_seed(0)
        logits = torch.randn(n, c, h, w, device=dev, generator=g)
        labels = torch.randint(0, c + 1, (n, h, w), device=dev, generator=g)
        labels[labels == c] = ignore
        counts = torch.zeros(c + 2, c + 1, device=dev, dtype=torch.int64)
        kernels = {"seg_ce": (lambda: K.seg_ce(logits, labels, None, ignore, "mean"), 8.0 * logits.numel() + 8.0 * labels.numel()),
                   "seg_confusion": (lambda: K.seg_confusion(logits, labels, c + 1, (), counts=counts), 4.0 * logits.numel() + 8.0 * labels.numel())}
        res = {}
        for _ in range(args.repeats):
            for name, (fn, _) in kernels.items():
                res.setdefault(name, []).append(timed(fn))
        for name, us in res.items():
            med, spread, nbytes = statistics.median(us), (max(us) - min(us)) / statistics.median(us), kernels[name][1]
            print(f"{n} x {c} x {h} x {w}  {name:14s} {med:9.1f} us (spread {spread:5.1%})  {nbytes * 1e-9:6.2f} GB  {nbytes / med * 1e-6:5.2f} TB/s of the "
                  f"algorithmic minimum ({nbytes / med * 1e-6 / HBM_TBS:5.1%} of HBM)")
        del logits, labels, counts, kernels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
