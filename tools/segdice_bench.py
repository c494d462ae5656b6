"""The region losses (csrc/seg_struct.h) at the Cityscapes recipe's logit map, 16 x 19 x 1024 x 2048, and BCEDiceLoss at
16 x 1 x 1024 x 2048, forward + backward, next to seg_ce and seg_ohem_ce on the same inputs and next to the same losses composed from plain
torch operations on the device (softmax, one-hot, products, sums and autograd through them: what a user had before these kernels).

    python tools/segdice_bench.py [--iters 10] [--repeats 3] [--batch 16]
Timed with device events after a warm-up, the calls interleaved inside every repeat; us per call is the median of --repeats runs with the
spread (max - min) / median.  GB is the ALGORITHMIC byte count - logits and labels (or the dense target) read twice, the gradient written once,
the same model as seg_ohem_ce's bar branch - and TB/s is that count over the time.  Measurement tool: product library only, needs the GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training.losses import BCEDiceLoss, DiceLoss

    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters  # us

    def fwd_bwd(crit, x, t):
        def run():
            x.grad = None
            crit(x, t).backward()
        return run

    def torch_dice(x, y, ignore):  # the reference's chain of ATen operations, C + 1 one-hot channels with the last one dropped
        p = x.softmax(1)
        t = F.one_hot(y, x.shape[1] + 1).permute(0, 3, 1, 2)[:, :ignore]
        v = (y != ignore).unsqueeze(1)
        inter, den = (t * p * v).sum((0, 2, 3)), ((t + p) * v).sum((0, 2, 3))
        return (1 - (2 * inter + 1.0) / (den + 1e-5 + 1.0)).mean()

    def torch_bce_dice(x, y):
        p, t = x.sigmoid(), y.unsqueeze(1).float()
        inter, den = (t * p).sum((0, 2, 3)), (t + p).sum((0, 2, 3))
        return 0.5 * F.binary_cross_entropy_with_logits(x, t) + 0.5 * (1 - (2 * inter + 1.0) / (den + 1e-5 + 1.0)).mean()

    n, c, h, w, ignore = args.batch, 19, 1024, 2048, 19
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(n, c, h, w, device=dev, generator=g).requires_grad_()
    labels = torch.randint(0, c + 1, (n, h, w), device=dev, generator=g)  # (the value c is the ignored label)
    x1 = torch.randn(n, 1, h, w, device=dev, generator=g).requires_grad_()
    y1 = torch.randint(0, 2, (n, h, w), device=dev, generator=g)
    multi = 2 * (4.0 * logits.numel() + 8.0 * labels.numel()) + 4.0 * logits.numel()
    binary = 2 * (4.0 * x1.numel() + 8.0 * y1.numel()) + 4.0 * x1.numel()
    calls = {"DiceLoss": (fwd_bwd(DiceLoss(ignore_index=ignore), logits, labels), multi),
             "DiceLoss in torch": (fwd_bwd(lambda a, b: torch_dice(a, b, ignore), logits, labels), multi),
             "seg_ce": (lambda: K.seg_ce(logits.detach(), labels, None, ignore, "mean"), None),
             "seg_ohem_ce bar": (lambda: K.seg_ohem_ce(logits.detach(), labels, 0.7, 0.1, ignore, False), multi),
             "BCEDiceLoss": (fwd_bwd(BCEDiceLoss(), x1, y1), binary),
             "BCEDiceLoss in torch": (fwd_bwd(torch_bce_dice, x1, y1), binary)}
    res = {}
    for _ in range(args.repeats):
        for name, (fn, _) in calls.items():
            res.setdefault(name, []).append(timed(fn))
    print(f"{n} x {c} x {h} x {w} (BCEDiceLoss: {n} x 1 x {h} x {w}), {args.iters} iterations, median of {args.repeats} repeats")
    med = {name: statistics.median(us) for name, us in res.items()}
    for name, us in res.items():
        nbytes = calls[name][1]
        traffic = f"  {nbytes / 1e9:5.2f} GB  {nbytes / med[name] / 1e6:5.2f} TB/s" if nbytes else ""
        print(f"{name:22s} {med[name]:9.1f} us (spread {(max(us) - min(us)) / med[name]:5.1%}){traffic}")
    for name in ("DiceLoss", "BCEDiceLoss"):
        print(f"{name}: {med[name + ' in torch'] / med[name]:.1f} x faster than the torch composition")


if __name__ == "__main__":
    main()
