"""TEST INFRASTRUCTURE ONLY: writes the fixtures of tests/test_sliding_window.py from the LIVE reference (needs the reference tree; run once,
in the build container):   python tests/make_sliding_window_golden.py

  tests/golden/sliding_window_tiles.json   inputs (h, w, tile_size, tile_step, min_tile_threshold) and what the reference's own
                                           SlidingWindowInferenceDetectionWrapper._generate_tiles returns for them: the (x, y) origins in order
                                           and the extent of the zero-padded image the tiles are views of
  tests/golden/sliding_window_merge.pt     a stub-model case: prepared decoded (boxes, scores) per tile, the wrapper parameters, and the rows the
                                           reference's own SlidingWindowInferenceDetectionWrapper.forward returns for them (torchvision's nms /
                                           batched_nms bound to oracle/nms.py, as oracle/ref_shim.py:273-280 does)
"""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden")

# (h, w, tile_size, tile_step, min_tile_threshold, what the case is)
TILE_CASES = [
    (128, 128, 64, 64, 30, "exact fit, step == size"),
    (128, 192, 64, 32, 30, "exact fit with overlap, non-square"),
    (148, 128, 64, 64, 30, "remainder 20 below the threshold: dropped"),
    (157, 128, 64, 64, 30, "remainder 29, one below the threshold: dropped"),
    (158, 128, 64, 64, 30, "remainder 30 at the threshold: padded"),
    (170, 200, 64, 64, 30, "remainders 42 / 8: rows padded, columns dropped"),
    (200, 170, 64, 48, 30, "overlap, remainders 40 / 10"),
    (300, 500, 128, 96, 30, "non-square with overlap, padding on both axes"),
    (2048, 2048, 640, 512, 30, "the throughput workload: 16 tiles"),
    (3000, 4000, 640, 512, 30, "a 12-megapixel image"),
    (40, 50, 64, 64, 30, "smaller than a tile on both axes (negative modulo)"),
    (40, 200, 64, 32, 30, "smaller than a tile on one axis"),
    (64, 64, 64, 64, 30, "exactly one tile"),
    (100, 100, 64, 64, 0, "threshold 0: every remainder padded"),
    (100, 100, 64, 64, 1000, "threshold above every remainder: never padded"),
]


def reference_wrapper_class():
    from oracle import nms as onms
    from oracle import ref_shim

    ref_shim.reference_post_prediction_callback(onms.nms, onms.batched_nms, score_threshold=0.5, nms_threshold=0.5, nms_top_k=10, max_predictions=10)
    import torchvision  # the stub: the wrapper calls torchvision.ops.boxes.batched_nms (:127)

    torchvision.ops.boxes.batched_nms = staticmethod(onms.batched_nms)
    from super_gradients.training.models.detection_models.sliding_window_detection_forward_wrapper import SlidingWindowInferenceDetectionWrapper

    return SlidingWindowInferenceDetectionWrapper


def tile_table(W):
    out = []
    for h, w, ts, step, thr, what in TILE_CASES:
        tiles = W._generate_tiles(types.SimpleNamespace(min_tile_threshold=thr), torch.zeros(1, 1, h, w), ts, step)
        ext = None
        if tiles:
            assert all(tuple(t.shape[-2:]) == (ts, ts) for t, _ in tiles)
            base = tiles[0][0]._base if tiles[0][0]._base is not None else tiles[0][0]
            ext = [int(base.shape[-2]), int(base.shape[-1])]
        out.append({"what": what, "h": h, "w": w, "tile_size": ts, "tile_step": step, "min_tile_threshold": thr,
                    "origins_xy": [[int(x), int(y)] for _, (x, y) in tiles], "padded_hw": ext})
    return out


def merge_case_inputs(seed=7, B=2, H=150, W=180, ts=64, step=48, L=48, C=3):
    """Clustered boxes in TILE coordinates: per image a few objects in image coordinates; every tile that sees one reports it several times
    (jittered, different scores), so both the tile stage and the merge have work; one tile of image 1 reports nothing."""
    g = torch.Generator().manual_seed(seed)
    origins = [(x, y) for y in (0, 48, 96) for x in (0, 48, 96)]  # what _generate_tiles gives for 150 x 180 / 64 / 48 / 30 (checked in main)
    T = len(origins)
    boxes = torch.zeros(B * T, L, 4)
    scores = torch.zeros(B * T, L, C)
    for b in range(B):
        centres = torch.rand(6, 2, generator=g) * torch.tensor([W * 1.0, H * 1.0])
        sizes = 14 + 20 * torch.rand(6, 2, generator=g)
        cls = torch.randint(0, C, (6,), generator=g)
        for t, (ox, oy) in enumerate(origins):
            for a in range(L):
                k = a % 6
                c = centres[k] + 1.5 * torch.randn(2, generator=g) - torch.tensor([ox * 1.0, oy * 1.0])
                s = sizes[k] * (1 + 0.05 * torch.randn(2, generator=g))
                inside = bool((c > 4).all() and (c < ts - 4).all())
                boxes[b * T + t, a] = torch.cat([c - s / 2, c + s / 2])
                if inside and not (b == 1 and t == 2):
                    scores[b * T + t, a, cls[k]] = 0.3 + 0.6 * torch.rand((), generator=g)
                    if a % 5 == 0:
                        scores[b * T + t, a, (cls[k] + 1) % C] = 0.25 + 0.2 * torch.rand((), generator=g)  # a second label on the same box
    scores = (scores * 64).round() / 64  # coarse scores: equal scores across tiles exercise the index tie rule
    return dict(B=B, H=H, W=W, tile_size=ts, tile_step=step, min_tile_threshold=30, T=T, boxes=boxes, scores=scores, conf=0.2, iou=0.5, nms_top_k=40,
                max_predictions=12)


class ReferenceStub(torch.nn.Module):
    """Returns the prepared decoded predictions of tile `call index` (the reference forwards image by image, tile by tile)."""

    def __init__(self, case, make_callback):
        super().__init__()
        self.case, self.make_callback, self.cursor = case, make_callback, 0

    def forward(self, tile):
        i, self.cursor = self.cursor, self.cursor + tile.shape[0]
        return (self.case["boxes"][i:self.cursor].to(tile.device), self.case["scores"][i:self.cursor].to(tile.device)), None

    def get_dataset_processing_params(self):
        return dict(class_names=None, image_processor=None, iou=None, conf=None, nms_top_k=None, max_predictions=None, multi_label_per_box=None,
                    class_agnostic_nms=None)

    def get_post_prediction_callback(self, *, conf, iou, nms_top_k, max_predictions, multi_label_per_box, class_agnostic_nms):
        return self.make_callback(score_threshold=conf, nms_threshold=iou, nms_top_k=nms_top_k, max_predictions=max_predictions,
                                  multi_label_per_box=multi_label_per_box, class_agnostic_nms=class_agnostic_nms)


def run_reference(W, case, class_agnostic):
    from oracle import nms as onms
    from oracle import ref_shim

    make = lambda **kw: ref_shim.reference_post_prediction_callback(onms.nms, onms.batched_nms, **kw)  # noqa: E731
    stub = ReferenceStub(case, make)
    wrapper = W(tile_size=case["tile_size"], tile_step=case["tile_step"], model=stub, min_tile_threshold=case["min_tile_threshold"],
                tile_nms_iou=case["iou"], tile_nms_conf=case["conf"], tile_nms_top_k=case["nms_top_k"], tile_nms_max_predictions=case["max_predictions"],
                tile_nms_multi_label_per_box=True, tile_nms_class_agnostic_nms=class_agnostic)
    with torch.no_grad():
        return [r.clone() for r in wrapper.forward(torch.zeros(case["B"], 3, case["H"], case["W"]))]


def main():
    W = reference_wrapper_class()
    with open(os.path.join(GOLDEN, "sliding_window_tiles.json"), "w") as f:
        json.dump({"source": "SlidingWindowInferenceDetectionWrapper._generate_tiles of the reference, called through oracle/ref_shim.py",
                   "cases": tile_table(W)}, f, indent=1)
    case = merge_case_inputs()
    grid = W._generate_tiles(types.SimpleNamespace(min_tile_threshold=30), torch.zeros(1, 1, case["H"], case["W"]), case["tile_size"], case["tile_step"])
    assert [xy for _, xy in grid] == [(x, y) for y in (0, 48, 96) for x in (0, 48, 96)] and len(grid) == case["T"]
    case["expected_per_class"] = run_reference(W, case, class_agnostic=False)
    case["expected_class_agnostic_tiles"] = run_reference(W, case, class_agnostic=True)
    torch.save(case, os.path.join(GOLDEN, "sliding_window_merge.pt"))
    print("tiles:", [len(c["origins_xy"]) for c in json.load(open(os.path.join(GOLDEN, "sliding_window_tiles.json")))["cases"]])
    print("merge rows per image:", [len(r) for r in case["expected_per_class"]], [len(r) for r in case["expected_class_agnostic_tiles"]])


if __name__ == "__main__":
    main()
