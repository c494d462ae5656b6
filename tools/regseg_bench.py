"""The RegSeg kernels (csrc/dilated.h, csrc/bilinear.h) at the model's own stage-3 shape: batch 16, 1024 x 2048 input -> 64 x 128 map, C = 256.

    python tools/regseg_bench.py [--iters 20] [--batch 16] [--repeats 3]
Timed with device events after a warm-up, the variants interleaved inside every repeat; us per call is the median of --repeats runs and the
spread (max - min) / median.
  (a) sgx_dgconv3x3_fwd / _bwd_data / _bwd_weight with dilations [1, 1] against sgx_gconv3x3_* on the same tensors: what the new staging costs
      where the old kernel also applies;
  (b) dilations [1, 4] (halo) and [1, 14] (band) against (a): what the band form costs;
  (c) the bilinear kernels: bytes moved per second against the algorithmic minimum (every operand once).
TFLOP/s from 2 * 9 * 16 * C * pixels against the 157 TFLOP/s fp32 matrix peak, TB/s against 6.3 TB/s.  Measurement tool: product library only."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS, MATRIX_TFS = 6.3, 157.0


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

    n, h, w, c, cg = args.batch, 64, 128, 256, 16
    x = torch.randn(n, h, w, c, device=dev)
    dy, y, dx = torch.randn_like(x), torch.empty_like(x), torch.empty_like(x)
    wt = torch.randn(c, cg, 3, 3, device=dev) / 12.0
    wk, halves = K.to_ohwi(wt), [K.to_ohwi(wt[: c // 2]), K.to_ohwi(wt[c // 2:])]
    dw, dhalves = K.ohwi_empty(c, cg, 3, 3, dev).zero_(), [K.ohwi_empty(c // 2, cg, 3, 3, dev).zero_() for _ in range(2)]
    conv = {"gconv": (lambda: K.gconv3x3_fwd(x, wk, c // cg, out=y, stat_partials=True), lambda: K.gconv3x3_bwd_data(dy, wk, c // cg, tuple(x.shape), out=dx),
                      lambda: K.gconv3x3_bwd_weight(x, dy, dw, c // cg))}
    for dil in ([1, 1], [1, 4], [1, 14]):
        conv[f"dgconv {dil} ({'/'.join(K.dgconv3x3_form(tuple(x.shape), cg, dil, s) for s in range(2))})"] = (
            lambda dil=dil: K.dgconv3x3_fwd(x, halves, cg, dil, out=y, stat_partials=True), lambda dil=dil: K.dgconv3x3_bwd_data(dy, halves, cg, dil, out=dx),
            lambda dil=dil: K.dgconv3x3_bwd_weight(x, dy, dhalves, cg, dil))
    # the decoder's x2 (align_corners) on the 128-channel projection at the stage-3 map, and the head's x4 to NCHW at 19 classes from a quarter-size map
    p2, up = torch.randn(n, h, w, 128, device=dev), torch.empty(n, 2 * h, 2 * w, 128, device=dev)
    dup, dp2 = torch.randn_like(up), torch.empty(n, h, w, 128, device=dev)
    logits = torch.randn(n, 256, 512, 19, device=dev)
    dmap = torch.randn(n, 19, 1024, 2048, device=dev)
    dlog = torch.empty_like(logits)
    sweeps = {"bilinear_fwd x2": (lambda: K.bilinear_fwd(p2, 2, True, out=up), p2.numel() + up.numel()),
              "bilinear_bwd x2": (lambda: K.bilinear_bwd(dup, 2, True, out=dp2), dup.numel() + dp2.numel()),
              "bilinear_nchw_fwd x4": (lambda: K.bilinear_nchw_fwd(logits, 4, False), logits.numel() + dmap.numel()),
              "bilinear_nchw_bwd x4": (lambda: K.bilinear_nchw_bwd(dmap, 4, False, out=dlog), logits.numel() + dmap.numel())}
    res = {}
    for _ in range(args.repeats):  # interleaved: every variant once per repeat
        for name, fns in conv.items():
            for p, fn in zip(("fwd", "dgrad", "wgrad"), fns):
                res.setdefault((name, p), []).append(timed(fn))
        for name, (fn, _) in sweeps.items():
            res.setdefault((name, ""), []).append(timed(fn))
    flop = 2.0 * 9 * cg * c * n * h * w
    print(f"batch {n}, map {h} x {w}, C {c}, group width {cg}; {args.iters} iterations, median of {args.repeats} repeats")
    for (name, p), us in res.items():
        med, spread = statistics.median(us), (max(us) - min(us)) / statistics.median(us)
        if p:
            nbytes = 4.0 * x.numel() * (3 if p == "wgrad" else 2)
            base = statistics.median(res[("gconv", p)])
            print(f"{name:34s} {p:6s} {med:9.1f} us (spread {spread:5.1%})  {flop / med * 1e-6:6.1f} TFLOP/s ({flop / med * 1e-6 / MATRIX_TFS:5.1%} of peak)  "
                  f"{nbytes / med * 1e-6:5.2f} TB/s ({nbytes / med * 1e-6 / HBM_TBS:5.1%})  x{med / base:4.2f} of gconv")
        else:
            nbytes = 4.0 * sweeps[name][1]
            print(f"{name:41s} {med:9.1f} us (spread {spread:5.1%})  {nbytes / med * 1e-6:5.2f} TB/s of the algorithmic minimum ({nbytes / med * 1e-6 / HBM_TBS:5.1%} of HBM)")


if __name__ == "__main__":
    main()
