"""beit_base_patch16_224 forward + backward on the chip, BEiT's glue kernels (csrc/vit.h) alone, and the attention kernels with the relative
position bias next to the plain ones at the same shape.

    python tools/beit_bench.py [--batch 64] [--size 224] [--steps 5] [--iters 10] [--rounds 3] [--model beit_base_patch16_224]
Part 1: images/s of one training forward + cross-entropy + backward of the model (device events after a warm-up, the median of --steps).
Part 2: every new kernel at the model's own shapes, timed alone (the median of --iters calls), with its HBM bound (algorithmic bytes at 8.0 TB/s)
and, for attention, its fp32 matrix bound (157.3 TFLOP/s; forward 4 T^2 d, backward 10 T^2 d flop per (image, head)); `calls` is how often the
step launches it, `ms/step` = calls x the time alone, `share` = that against the step of part 1.
Part 3: sgx_attn_rpb_fwd / _bwd against sgx_attn_fwd / _bwd, interleaved (plain, bias, plain, bias, ... --rounds times, one process): the medians,
the spread of each over the rounds and the ratio.  Measurement tool: product library only."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="beit_base_patch16_224")
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

    blk = net.blocks[0]
    depth, heads, D = len(net.blocks), blk.attn.num_heads, net.embed_dim
    grid = net.patch_embed.grid_size
    d, T, N = D // heads, grid[0] * grid[1] + 1, K.rpb_rows(grid)
    scale = d ** -0.5
    rnd = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    xs, dy, t = rnd(B, T, 1, D), rnd(B, T, 1, D), rnd(B, T, 1, D)
    gamma, dgam = rnd(D), torch.zeros(D, device=dev)
    m = (torch.rand(B, device=dev) < 0.9).float() / 0.9
    qkv, dqkv = rnd(B, T, 1, 3 * D), torch.empty(B, T, 1, 3 * D, device=dev)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    table, dtable = rnd(N, heads), torch.zeros(N, heads, device=dev)
    o, lse = K.attn_rpb_fwd(q, k, v, heads, scale, table, grid)
    o0, lse0 = K.attn_fwd(q, k, v, heads, scale)
    pooled = rnd(B, 1, 1, D)
    patch, cls, dcls = rnd(B, T - 1, 1, D), rnd(D), torch.zeros(D, device=dev)
    tok = 4.0 * B * T * D  # bytes of one [B, T, D] map
    att = B * heads * float(T) * T * d
    dq, dk, dv = dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:]
    rpb_fwd = lambda: K.attn_rpb_fwd(q, k, v, heads, scale, table, grid)  # noqa: E731
    rpb_bwd = lambda: K.attn_rpb_bwd(q, k, v, o, dy, lse, heads, scale, table, grid, dq, dk, dv, dtable)  # noqa: E731
    plain_fwd = lambda: K.attn_fwd(q, k, v, heads, scale)  # noqa: E731
    plain_bwd = lambda: K.attn_bwd(q, k, v, o0, dy, lse0, heads, scale, dq, dk, dv)  # noqa: E731
    rows = [
        ("attn_rpb_fwd", rpb_fwd, depth, 4 * tok, 4 * att),
        ("attn_rpb_bwd (+dtable)", rpb_bwd, depth, 8 * tok, 10 * att),
        ("layerscale_fwd (gamma)", lambda: K.layerscale_fwd(xs, t, gamma), 2 * depth, 3 * tok, 0.0),
        ("layerscale_fwd (gamma, m)", lambda: K.layerscale_fwd(xs, t, gamma, m), 0, 3 * tok, 0.0),
        ("layerscale_bwd (gamma, dgamma)", lambda: K.layerscale_bwd(dy, t, gamma, None, dgam), 2 * depth, 3 * tok, 0.0),
        ("layerscale_bwd (gamma, m, dgamma)", lambda: K.layerscale_bwd(dy, t, gamma, m, dgam), 0, 3 * tok, 0.0),
        ("token_mean_fwd", lambda: K.token_mean_fwd(xs), 1, tok, 0.0),
        ("token_mean_bwd", lambda: K.token_mean_bwd(pooled, T), 1, tok, 0.0),
        ("token_assemble_fwd (no pos)", lambda: K.token_assemble_fwd(patch, cls, None), 1, 2 * tok, 0.0),
        ("token_assemble_bwd (no pos)", lambda: K.token_assemble_bwd(dy, dcls, None), 1, tok / T, 0.0),
    ]
    print(f"{'kernel':<42}{'us alone':>10}{'spread':>8}{'HBM bound us':>14}{'of bound':>10}{'matrix bound us':>17}{'calls':>7}{'ms/step':>9}{'share':>8}")
    for name, fn, calls, nbytes, flop in rows:
        tm, sp = timed(fn, args.iters)
        hb, mb = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        bound = max(hb, mb)
        print(f"{name:<42}{tm * 1e3:>10.1f}{sp:>8.1%}{hb:>14.1f}{bound / (tm * 1e3):>10.1%}{mb:>17.1f}{calls:>7}{calls * tm:>9.2f}{calls * tm / ms:>8.1%}")

    res = {"attn_fwd": [], "attn_rpb_fwd": [], "attn_bwd": [], "attn_rpb_bwd": []}
    for _ in range(args.rounds):
        for name, fn in (("attn_fwd", plain_fwd), ("attn_rpb_fwd", rpb_fwd), ("attn_bwd", plain_bwd), ("attn_rpb_bwd", rpb_bwd)):
            res[name].append(timed(fn, args.iters)[0])
    med = {k_: statistics.median(v_) for k_, v_ in res.items()}
    print(f"with the bias against the plain kernels, B {B}, heads {heads}, T {T}, d {d}, N {N} (interleaved, {args.rounds} rounds of the median of {args.iters}):")
    for plain, bias in (("attn_fwd", "attn_rpb_fwd"), ("attn_bwd", "attn_rpb_bwd")):
        sp = {k_: (max(res[k_]) - min(res[k_])) / med[k_] for k_ in (plain, bias)}
        print(f"  {plain} {med[plain] * 1e3:.1f} us (spread over rounds {sp[plain]:.1%}), {bias} {med[bias] * 1e3:.1f} us (spread {sp[bias]:.1%}): ratio {med[bias] / med[plain]:.3f}")


if __name__ == "__main__":
    main()
