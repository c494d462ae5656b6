"""Measure every arena optimizer's step over one arena, interleaved with sgx_adamw_step from the same library in the same process.

    python tools/optim_bench.py [--n 12900000] [--slots 534] [--reps 100] [--inner 10] [--warmup 20] [--out profiles/<name>.json]

Prints one JSON line: per optimizer the median / min time of a step (HIP events around `inner` back-to-back steps, `reps` such windows taken round-robin over
the optimizers so that clock and memory state are shared), the algorithmic bytes per element and the achieved bytes/s.  The arena is
synthetic: `n` elements (default: the 12.9 M parameters of YOLO-NAS-S) cut into `slots` tensors of log-uniform sizes, every third one
without weight decay (so the weight-decay table has as many segments as slots: harder than a model's, where neighbours merge).  Algorithmic bytes per element: every arena read once and written once per pass (fp32) -
AdamW / Adam 28 (p, g, m, v in; p, m, v out), Lion 20, RMSprop 20 + 8 per enabled buffer, SGD momentum 20,
Lamb 44 = 4 (gradient-norm pre-pass) + 24 (moments: p, g, m, v in; m, v out) + 16 (apply: p, m, v in; p out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12_900_000)
    ap.add_argument("--slots", type=int, default=534)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back steps inside one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from super_gradients_amd import kernels as K

    dev = torch.device("cuda:0")
    g_ = torch.Generator().manual_seed(0)
    w = torch.exp(torch.rand(a.slots, generator=g_) * 9.0)
    sizes = torch.clamp((w / w.sum() * a.n).long() // 64 * 64, min=64)  # 64-element aligned slots, as modules/engine.py lays them out
    slot_end = torch.cumsum(sizes, 0)
    n = int(slot_end[-1])
    seg_end = slot_end.clone().to(dev)
    seg_wd = torch.tensor([0.0 if i % 3 == 0 else 1e-5 for i in range(a.slots)], dtype=torch.float32, device=dev)
    slot_end = slot_end.to(dev)
    z = lambda v=0.0: torch.full((n,), v, dtype=torch.float32, device=dev)  # noqa: E731
    p, g = torch.randn(n, device=dev) * 0.1, torch.randn(n, device=dev) * 1e-3
    m, v, s3, ga = z(), z(), z(), z()
    sq = z(1.0)
    ws, trust = K.lamb_workspace(n, a.slots, dev), torch.ones(a.slots, device=dev)
    step = [0]
    runs = {
        "AdamW": (28, lambda: K.adamw_step(p, g, m, v, 2e-4, 0.9, 0.999, 1e-8, step[0], seg_end, seg_wd)),
        "Adam": (28, lambda: K.adam_step(p, g, m, v, 2e-4, 0.9, 0.999, 1e-8, step[0], seg_end, seg_wd)),
        "Lion": (20, lambda: K.lion_step(p, g, m, 1e-5, 0.9, 0.99, seg_end, seg_wd)),
        "RMSprop": (20, lambda: K.rmsprop_step(p, g, sq, None, None, 1e-4, 0.99, 1e-8, 0.0, seg_end, seg_wd)),
        "RMSpropTF_centered_momentum": (36, lambda: K.rmsprop_step(p, g, sq, ga, s3, 1e-4, 0.9, 1e-10, 0.9, seg_end, seg_wd, tf=True, lr_in_momentum=True)),
        "SGD_momentum": (20, lambda: K.sgd_step(p, g, s3, 1e-4, 0.9, 0.0, False, False, seg_end, seg_wd)),
        "Lamb": (44, lambda: K.lamb_step(p, g, m, v, 1e-4, 0.9, 0.999, 1e-6, step[0], seg_end, seg_wd, slot_end, ws, trust)),
    }
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.reps):
        step[0] += 1
        for name, (_, fn) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    assert bool(torch.isfinite(p).all())
    res = {"tool": "optim_bench", "device": torch.cuda.get_device_name(0), "n": n, "slots": a.slots, "reps": a.reps, "inner": a.inner, "optimizers": {}}
    for name, (bpe, _) in runs.items():
        med = statistics.median(times[name])
        res["optimizers"][name] = {"median_us": round(med, 2), "min_us": round(min(times[name]), 2), "bytes_per_element": bpe,
                                   "tb_per_s": round(bpe * n / med / 1e6, 3)}
    res["lamb_over_adamw"] = round(res["optimizers"]["Lamb"]["median_us"] / res["optimizers"]["AdamW"]["median_us"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
