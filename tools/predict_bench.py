"""predict() throughput on one GPU: YOLO-NAS-S (random-init, 80 classes), the reference's default COCO processing (longest side -> 636, centre pad
to 640x640 with 114, /255), batches of 32 synthetic 480x640 uint8 images already resident in HBM.  Prints one JSON line with the end-to-end
rate and the split pre-processing launch / fused eval forward / NMS (HIP events).  Usage: python tools/predict_bench.py [--batches 10]

--sliding-window: the tiled path instead (SlidingWindowInferenceDetectionWrapper.predict, skip_image_resizing=True) on 8 uint8 images of
2048 x 2048, tile 640, step 512 (16 tiles per image), against the reference-shaped loop built from the pieces that exist without the
wrapper: per image and tile a slice of the zero-padded pre-processed tensor, a batch-1 forward of the same fused model, the callback per
tile, the shift by the tile origin, a host concatenation and a CPU merge (oracle/nms.py's batched_nms, the restatement of torchvision's).
Both run in this process, interleaved round by round; the medians over the rounds and their ratio are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--model", default="s", choices=["s", "m", "l"])
    ap.add_argument("--family", default="yolo_nas", choices=["yolo_nas", "ppyoloe"], help="ppyoloe: PP-YOLOE with the reference's default COCO processing "
                    "(reverse channels, rescale to 640x640, normalise)")
    ap.add_argument("--fp32", action="store_true", help="predict(fp16=False): the fp32 path (default: the reference's default fp16=True -> bf16 kernels)")
    ap.add_argument("--tile", type=int, nargs=3, default=None, metavar=("BM", "BN", "KD"), help="force the bf16 conv kernel's tile / slab depth (0 = heuristic)")
    ap.add_argument("--sliding-window", action="store_true", help="the tiled path on 2048 x 2048 images against the reference-shaped per-tile loop")
    ap.add_argument("--rounds", type=int, default=5, help="--sliding-window: interleaved rounds (one batch of each path per round)")
    a = ap.parse_args()
    if a.sliding_window:
        return sliding_window(a)
    from super_gradients_amd.training import models
    from super_gradients_amd.training.processing import default_ppyoloe_coco_processing_params, default_yolo_nas_coco_processing_params

    dev = torch.device("cuda:0")
    net = models.get(f"{a.family}_{a.model}", num_classes=80).materialize(dev)
    if a.tile:
        from super_gradients_amd._lib import check, lib

        check(lib().sgx_hconv_debug_set_tile(*a.tile), "sgx_hconv_debug_set_tile")
    net.set_dataset_processing_params(**(default_ppyoloe_coco_processing_params() if a.family == "ppyoloe" else default_yolo_nas_coco_processing_params()))
    g = torch.Generator(device="cpu").manual_seed(0)
    images = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(a.batch)]
    pipe = net._get_pipeline(conf=0.01, fp16=not a.fp32)
    pipe(images, batch_size=a.batch)  # warm-up: fuses the model copy
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    split = [0.0, 0.0, 0.0]
    t0 = time.perf_counter()
    for _ in range(a.batches):
        ev[0].record()
        batch, metas = pipe.image_processor.preprocess_batch(images, device=dev)
        ev[1].record()
        with torch.no_grad():
            out = pipe.model(batch)
        ev[2].record()
        rows = pipe.post_prediction_callback(out, device=dev)
        ev[3].record()
        torch.cuda.synchronize()
        for i in range(3):
            split[i] += ev[i].elapsed_time(ev[i + 1])
    t_stage = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(a.batches):
        res = pipe(images, batch_size=a.batch)
    torch.cuda.synchronize()
    t_e2e = time.perf_counter() - t0
    n = a.batches * a.batch
    gmac = {"s": 16.939, "m": 47.093, "l": 64.493}[a.model] if a.family == "yolo_nas" else {"s": 8.7, "m": 24.9, "l": 55.0}[a.model]  # forward GMAC per 640 x 640 image (PP-YOLOE: the paper's FLOPs / 2)
    fwd_ms = split[1] / a.batches
    print(json.dumps({"metric": "images/s %s-%s predict() 480x640 -> 640x640, bs=%d, %s, fused blocks" % ("PP-YOLOE" if a.family == "ppyoloe" else "YOLO-NAS", a.model.upper(), a.batch, "bf16" if pipe.half else "fp32"),
                      "value": round(n / t_e2e, 1), "dtype": "bf16 (fp32 accumulate, fp32 prediction outputs)" if pipe.half else "fp32", "tile_override": a.tile,
                      "forward_tflops": round(2 * gmac * a.batch / fwd_ms, 1),
                      "end_to_end_includes": "device pre-processing, eval forward, NMS, D2H of the kept rows, host box post-processing, result objects",
                      "ms_per_batch": {"preprocess": round(split[0] / a.batches, 3), "forward": round(split[1] / a.batches, 3),
                                       "nms": round(split[2] / a.batches, 3), "stages_wall": round(1e3 * t_stage / a.batches, 3),
                                       "end_to_end": round(1e3 * t_e2e / a.batches, 3)},
                      "detections_first_image": len(res[0].prediction), "data": "synthetic uint8 images resident in HBM, random-init weights"}))


def sliding_window(a):
    import statistics

    from oracle import nms as onms
    from super_gradients_amd.training import models
    from super_gradients_amd.training.models.detection_models.sliding_window_detection_forward_wrapper import SlidingWindowInferenceDetectionWrapper
    from super_gradients_amd.training.processing import default_yolo_nas_coco_processing_params

    dev = torch.device("cuda:0")
    B, S, tile, step = 8, 2048, 640, 512
    net = models.get(f"yolo_nas_{a.model}", num_classes=80).materialize(dev)
    net.set_dataset_processing_params(**default_yolo_nas_coco_processing_params())
    wrapper = SlidingWindowInferenceDetectionWrapper(tile_size=tile, tile_step=step, model=net)
    g = torch.Generator(device="cpu").manual_seed(0)
    images = [torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    kw = dict(conf=0.01, fp16=not a.fp32, skip_image_resizing=True)
    pipe = wrapper._get_pipeline(**kw)
    res = pipe(images, batch_size=B)  # warm-up: fuses the model copy
    fused, cb = pipe.model.model, pipe.post_prediction_callback
    origins, ph, pw = wrapper._tile_grid(S, S)
    T = len(origins)

    def loop():
        batch, metas = pipe.image_processor.preprocess_batch(images, device=dev)
        out = []
        with torch.no_grad():
            for b in range(B):
                img = batch[b:b + 1]
                padded = torch.zeros(1, img.shape[1], ph, pw, device=dev)
                padded[:, :, :S, :S] = img
                dets = []
                for x, y in origins:
                    for r in cb(fused(padded[:, :, y:y + tile, x:x + tile]), device=dev):
                        if len(r):
                            r = r.clone()
                            r[:, :4] += torch.tensor([x, y, x, y], device=dev)
                            dets.append(r)
                if dets:
                    d = torch.cat(dets).cpu()
                    out.append(d[onms.batched_nms(d[:, :4], d[:, 4], d[:, 5], cb.nms_threshold)])
                else:
                    out.append(torch.zeros(0, 6))
        return out

    base = loop()  # warm-up of the batch-1 shapes
    same = all(len(r.prediction) == len(q) for r, q in zip(res, base))
    t_tiled, t_loop = [], []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pipe(images, batch_size=B)
        torch.cuda.synchronize()
        t_tiled.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        base = loop()
        torch.cuda.synchronize()
        t_loop.append(time.perf_counter() - t0)
    mt, ml = statistics.median(t_tiled), statistics.median(t_loop)
    print(json.dumps({"metric": "images/s YOLO-NAS-%s sliding-window predict() 2048x2048, tile 640, step 512 (16 tiles), bs=%d, %s" % (a.model.upper(), B, "bf16" if pipe.half else "fp32"),
                      "value": round(B / mt, 2), "tiles_per_s": round(B * T / mt, 1), "loop_images_per_s": round(B / ml, 2), "loop_tiles_per_s": round(B * T / ml, 1),
                      "ratio_tiled_over_loop": round(ml / mt, 2), "rounds": a.rounds, "tiled_s": [round(t, 4) for t in t_tiled], "loop_s": [round(t, 4) for t in t_loop],
                      "merged_rows_first_image": len(res[0].prediction), "loop_rows_first_image": len(base[0]), "row_counts_agree": same,
                      "loop": "per tile: slice of the zero-padded batch, batch-1 forward of the same fused model, callback, shift; host concatenation; CPU merge (oracle/nms.py)",
                      "data": "synthetic uint8 images resident in HBM, random-init weights"}))


if __name__ == "__main__":
    main()
