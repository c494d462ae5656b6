"""vit_base forward + backward on the chip, and the Vision Transformer's glue kernels (csrc/vit.h) alone against their bounds.

    python tools/vit_bench.py [--batch 64] [--size 224] [--steps 5] [--iters 10] [--model vit_base]
Part 1: images/s of one training forward + cross-entropy + backward of the model (device events after a warm-up, the median of --steps).
Part 2: every new kernel at the model's own shapes, timed alone (the median of --iters calls), with its HBM bound (algorithmic bytes at
8.0 TB/s) and, for attention, its fp32 matrix bound (157.3 TFLOP/s; forward 4 T^2 d, backward 10 T^2 d flop per (image, head)); `calls` is how
often the step launches it, `ms/step` = calls x the time alone, `share` = that against the step of part 1.  What the rows leave of the step is
the token-wise linear layers (1x1 convolutions and their weight / data gradients), the head and the loss.  Measurement tool: product library only."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM, MATRIX = 8.0e12, 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--model", default="vit_base")
    args = ap.parse_args()
    import torch

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training import models
    from super_gradients_amd.training.losses import CrossEntropyLoss

    dev = torch.device("cuda:0")

    def timed(fn, n, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out), (max(out) - min(out)) / statistics.median(out)

    torch.manual_seed(0)
    net = models.get(args.model, arch_params=dict(image_size=(args.size, args.size)), num_classes=1000)
    net.materialize(dev).train()
    B = args.batch
    x = torch.randn(B, 3, args.size, args.size, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)
    loss_fn = CrossEntropyLoss()

    def step():
        net.zero_grad()
        loss_fn(net(x), y).backward()

    ms, spread = timed(step, args.steps)
    print(f"{args.model} forward + backward, batch {B}, {args.size} x {args.size}: {ms:.2f} ms/step, {B / ms * 1e3:.1f} images/s (median of {args.steps}, spread {spread:.1%})")

    blk = net.transformer.blocks[0]
    depth, heads, D = len(net.transformer.blocks), blk.attn.heads, net.hidden_dim
    d, F_, T = D // heads, blk.mlp.fc1.out_features, net.pos_embedding.shape[1]
    ph, pw = net.patch_size
    rnd = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    xs, dy, add = rnd(B, T, 1, D), rnd(B, T, 1, D), rnd(B, T, 1, D)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    _, mean, rstd = K.layernorm_fwd(xs, gamma, beta, 1e-6)
    dgam, dbet = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    qkv, dqkv = rnd(B, T, 1, 3 * D), torch.empty(B, T, 1, 3 * D, device=dev)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    o, lse = K.attn_fwd(q, k, v, heads, d ** -0.5)
    h, dh = rnd(B, T, 1, F_), rnd(B, T, 1, F_)
    img = rnd(B, args.size, args.size, 4)
    patch = rnd(B, T - 1, 1, D)
    cls, pos, dcls, dpos = rnd(D), rnd(T, D), torch.zeros(D, device=dev), torch.zeros(T, D, device=dev)
    tok, ftok = 4.0 * B * T * D, 4.0 * B * T * F_  # bytes of one [B, T, D] / [B, T, F] map
    att = B * heads * float(T) * T * d
    rows = [
        ("layernorm_fwd", lambda: K.layernorm_fwd(xs, gamma, beta, 1e-6), 2 * depth, 2 * tok, 0.0),
        ("layernorm_bwd (+addend, dgamma, dbeta)", lambda: K.layernorm_bwd(dy, xs, gamma, mean, rstd, dgam, dbet, addend=add), 2 * depth, 6 * tok, 0.0),
        ("gelu_fwd", lambda: K.gelu_fwd(h), 2 * depth, 2 * ftok, 0.0),
        ("gelu_bwd", lambda: K.gelu_bwd(dh, h, out=dh), depth, 3 * ftok, 0.0),
        ("attn_fwd", lambda: K.attn_fwd(q, k, v, heads, d ** -0.5), depth, 4 * tok, 4 * att),
        ("attn_bwd", lambda: K.attn_bwd(q, k, v, o, dy, lse, heads, d ** -0.5, dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:]), depth, 8 * tok, 10 * att),
        ("patch_rows", lambda: K.patch_rows(img, ph, pw), 1, 2 * 4.0 * img.numel(), 0.0),
        ("token_assemble_fwd", lambda: K.token_assemble_fwd(patch, cls, pos), 1, 2 * tok, 0.0),
        ("token_assemble_bwd", lambda: K.token_assemble_bwd(dy, dcls, dpos), 1, tok, 0.0),
    ]
    print(f"{'kernel':<42}{'us alone':>10}{'spread':>8}{'HBM bound us':>14}{'of bound':>10}{'matrix bound us':>17}{'calls':>7}{'ms/step':>9}{'share':>8}")
    total = {}
    for name, fn, calls, nbytes, flop in rows:
        t, sp = timed(fn, args.iters)
        hb, mb = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        bound = max(hb, mb)
        total[name.split("_")[0].split(" ")[0]] = total.get(name.split("_")[0].split(" ")[0], 0.0) + calls * t
        print(f"{name:<42}{t * 1e3:>10.1f}{sp:>8.1%}{hb:>14.1f}{bound / (t * 1e3):>10.1%}{mb:>17.1f}{calls:>7}{calls * t:>9.2f}{calls * t / ms:>8.1%}")
    print("per kernel class, ms/step and share of the step: " + ", ".join(f"{k} {v:.2f} ({v / ms:.1%})" for k, v in total.items()) +
          f"; linear layers, head, loss and the rest {ms - sum(total.values()):.2f} ({1 - sum(total.values()) / ms:.1%})")


if __name__ == "__main__":
    main()
