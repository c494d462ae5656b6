"""Sliding-window (tiled) detection inference: the tile grid, the device tile gather, the cross-tile merge kernel, the wrapper and its
predict() pipeline (reference: sliding_window_detection_forward_wrapper.py, pipelines.py:373-395).  Kernel tests take the `backend`
fixture: the host emulation of the same kernel sources without a GPU, the product library on the chip."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import nms as onms
from oracle import ref_shim
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _wrapper_cls():
    from super_gradients_amd.training.models.detection_models.sliding_window_detection_forward_wrapper import SlidingWindowInferenceDetectionWrapper

    return SlidingWindowInferenceDetectionWrapper


def oracle_merge(tile_rows, origins, T, iou):
    """The composition the merge kernel replaces: per image, concatenate the tiles' rows in tile order, add the tile origin in fp32,
    oracle.nms.batched_nms (torchvision's CPU arithmetic), index.  tile_rows: B*T tensors [n, 6] (CPU).  -> B tensors [Ni, 6]"""
    out = []
    for b in range(len(tile_rows) // T):
        parts = []
        for t in range(T):
            r = tile_rows[b * T + t].clone().float()
            if len(r):
                x, y = origins[t]
                r[:, :4] = r[:, :4] + torch.tensor([x, y, x, y], dtype=torch.float32)
                parts.append(r)
        if not parts:
            out.append(torch.zeros(0, 6))
            continue
        d = torch.cat(parts)
        out.append(d[onms.batched_nms(d[:, :4], d[:, 4], d[:, 5], iou)])
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the tile grid
def test_tile_grid_matches_reference_table():
    """_tile_grid against the table the reference's own _generate_tiles produced (tests/make_sliding_window_golden.py)."""
    with open(os.path.join(GOLDEN, "sliding_window_tiles.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 12
    W = _wrapper_cls()
    for c in cases:
        w = W.__new__(W)
        w.tile_size, w.tile_step, w.min_tile_threshold = c["tile_size"], c["tile_step"], c["min_tile_threshold"]
        origins, ph, pw = W._tile_grid(w, c["h"], c["w"])
        assert [list(o) for o in origins] == c["origins_xy"], c["what"]
        if c["padded_hw"] is not None:
            assert [ph, pw] == c["padded_hw"], c["what"]


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_tile_table_fixture_matches_live_reference():
    import make_sliding_window_golden as G

    with open(os.path.join(GOLDEN, "sliding_window_tiles.json")) as f:
        assert json.load(f)["cases"] == G.tile_table(G.reference_wrapper_class())


# ---------------------------------------------------------------------------------------------------------------- 2. the gather
@pytest.mark.parametrize("dtype,C", [(torch.float32, 4), (torch.float32, 64), (torch.bfloat16, 8), (torch.bfloat16, 48)])
@pytest.mark.parametrize("H,W,tile,step", [(100, 90, 32, 24), (64, 96, 32, 32)])
def test_tile_gather_is_a_zero_padded_slice(backend, dtype, C, H, W, tile, step):
    """torch.equal to slicing a zero-padded copy: fp32 and bf16, the first convolution's channel padding and a wide C, a grid with padding
    on both axes (100 x 90: remainders 20 / 10, threshold 5) and an exact fit with step == size, B > 1."""
    from super_gradients_amd import kernels as K

    Wc = _wrapper_cls()
    w = Wc.__new__(Wc)
    w.tile_size, w.tile_step, w.min_tile_threshold = tile, step, 5
    origins, ph, pw = Wc._tile_grid(w, H, W)
    if (H, W) == (100, 90):
        assert ph > H and pw > W
    B, T = 3, len(origins)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    padded = torch.zeros(B, ph, pw, C, dtype=dtype)
    padded[:, :H, :W] = x
    want = torch.stack([padded[b, oy:oy + tile, ox:ox + tile] for b in range(B) for ox, oy in origins])
    got = K.tile_gather(x.to(backend), torch.tensor(origins, dtype=torch.int32).to(backend), tile).cpu()
    assert got.shape == (B * T, tile, tile, C) and got.dtype == dtype
    assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 3. the merge
def _clustered_rows(seed, B, T, P, origins, tile, n_objects, n_classes, fill, empty_tiles=(), empty_images=(), coarse_scores=False):
    """Post-NMS-shaped tile rows: objects live in image coordinates, a tile reports (jittered copies of) the objects it sees in its own
    coordinates, so overlapping tiles report the same object and boxes of different classes overlap.  fill: rows per tile (<= P)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(B * T, P, 6)
    counts = torch.zeros(B * T, dtype=torch.int32)
    span = max(max(o) for o in origins) + tile
    for b in range(B):
        centres = torch.rand(n_objects, 2, generator=g) * span
        sizes = 10 + 30 * torch.rand(n_objects, 2, generator=g)
        cls = torch.randint(0, n_classes, (n_objects,), generator=g)
        for t, (ox, oy) in enumerate(origins):
            if b in empty_images or (b, t) in empty_tiles:
                continue
            n = fill if isinstance(fill, int) else int(fill[(b * T + t) % len(fill)])
            k = torch.randint(0, n_objects, (n,), generator=g)
            c = centres[k] + 2.0 * torch.randn(n, 2, generator=g) - torch.tensor([float(ox), float(oy)])
            s = sizes[k] * (1 + 0.1 * torch.randn(n, 2, generator=g))
            sc = 0.05 + 0.9 * torch.rand(n, generator=g)
            if coarse_scores:
                sc = (sc * 16).round() / 16
            sc = torch.sort(sc, descending=True).values  # (NMS rows come sorted by score)
            rows[b * T + t, :n] = torch.cat([c - s / 2, c + s / 2, sc[:, None], cls[k, None].float()], 1)
            counts[b * T + t] = n
    return rows, counts


def _check_merge(backend, rows, counts, origins, T, iou):
    from super_gradients_amd import kernels as K

    out, cnt = K.tile_merge(rows.to(backend), counts.to(backend), torch.tensor(origins, dtype=torch.int32).to(backend), T, iou)
    out, cnt = out.cpu(), cnt.cpu()
    want = oracle_merge([rows[i, :int(counts[i])] for i in range(rows.shape[0])], origins, T, iou)
    assert out.shape == (rows.shape[0] // T, T * rows.shape[1], 6)
    for b, w in enumerate(want):
        assert int(cnt[b]) == len(w), (b, int(cnt[b]), len(w))
        assert torch.equal(out[b, :len(w)].view(torch.int32), w.view(torch.int32)), b
        assert not out[b, len(w):].any()
    return [len(w) for w in want], [int(counts[b * T:(b + 1) * T].sum()) for b in range(len(want))]


_GRID9 = [(x, y) for y in (0, 48, 96) for x in (0, 48, 96)]    # tile 64, step 48: overlapping tiles
_GRID16 = [(x, y) for y in range(0, 2048, 512) for x in range(0, 2048, 512)]  # the 2048 x 2048 / 640 / 512 workload


def test_merge_offset_form_below_1000(backend):
    """merged counts below 1000 (4 n <= 4000: the coordinate-offset form), tiles with count 0, an image whose tiles are all empty, the same
    object seen by overlapping tiles, several classes with overlapping boxes, equal scores across tiles (the index tie rule)."""
    rows, counts = _clustered_rows(1, 3, 9, 40, _GRID9, 64, n_objects=7, n_classes=3, fill=[40, 25, 0, 33], empty_tiles={(0, 4)}, empty_images={1},
                                   coarse_scores=True)
    kept, merged = _check_merge(backend, rows, counts, _GRID9, 9, 0.5)
    assert merged[1] == 0 and kept[1] == 0 and 0 < merged[0] < 1000 and 0 < kept[0] < merged[0]
    flat = rows[:9][:, :, 4][rows[:9][:, :, 4] > 0]
    assert len(flat.unique()) < len(flat)  # equal scores do occur


def test_merge_two_tiles_report_one_object(backend):
    """one object reported by two overlapping tiles: the lower score goes; the same box under another class stays; equal scores: lower index wins"""
    origins = [(0, 0), (48, 0)]
    rows = torch.zeros(2, 4, 6)
    rows[0, 0] = torch.tensor([50., 10., 62., 30., 0.9, 1.])  # image frame: 50..62
    rows[1, 0] = torch.tensor([2., 10., 14., 30., 0.8, 1.])   # the same place seen from tile 1: suppressed
    rows[1, 1] = torch.tensor([2., 10., 14., 30., 0.8, 2.])   # same box, another class: kept
    rows[0, 1] = torch.tensor([20., 40., 30., 60., 0.5, 0.])
    rows[1, 2] = torch.tensor([-28., 40., -18., 60., 0.5, 0.])  # equal score, same place: the earlier merged index (tile 0) wins
    counts = torch.tensor([2, 3], dtype=torch.int32)
    kept, _ = _check_merge(backend, rows, counts, origins, 2, 0.5)
    assert kept == [3]


@pytest.mark.parametrize("fill,what", [(112, "1008 merged rows: between torchvision's 1000-candidate switch and 1024"),
                                       ([150, 100, 140], "above 1024")])
def test_merge_per_class_form(backend, fill, what):
    rows, counts = _clustered_rows(2, 2, 9, 150, _GRID9, 64, n_objects=40, n_classes=4, fill=fill)
    kept, merged = _check_merge(backend, rows, counts, _GRID9, 9, 0.6)
    assert all(m > 1000 for m in merged), what
    if isinstance(fill, int):
        assert all(1000 < m <= 1024 for m in merged)
    else:
        assert all(m > 1024 for m in merged)


def test_merge_near_4800_rows(backend):
    """16 tiles x 300 rows: past the 1024-candidate LDS form and the 4096-key sort of the per-image kernel"""
    rows, counts = _clustered_rows(3, 2, 16, 300, _GRID16, 640, n_objects=400, n_classes=5, fill=[300, 300, 298, 300, 295])
    kept, merged = _check_merge(backend, rows, counts, _GRID16, 16, 0.7)
    assert all(4700 < m <= 4800 for m in merged) and all(0 < k < m for k, m in zip(kept, merged))


def test_merge_above_the_limit_is_an_argument_error(backend):
    from super_gradients_amd import _lib
    from super_gradients_amd import kernels as K

    assert K.TILE_MERGE_MAX_ROWS >= 8192
    with open(os.path.join(HERE, "..", "include", "sgx_hip.h")) as f:
        assert f"#define SGX_TILE_MERGE_MAX_ROWS {K.TILE_MERGE_MAX_ROWS}\n" in f.read()
    T, P = 64, K.TILE_MERGE_MAX_ROWS // 64 + 1
    origins = torch.zeros(T, 2, dtype=torch.int32, device=backend)
    with pytest.raises(_lib.SgxError, match="status -1"):
        K.tile_merge(torch.zeros(T, P, 6, device=backend), torch.zeros(T, dtype=torch.int32, device=backend), origins, T, 0.5)
    rows, counts = _clustered_rows(4, 1, 64, 256, [(8 * i, 0) for i in range(64)], 64, n_objects=30, n_classes=2, fill=[3, 0, 5])
    _check_merge(backend, rows, counts, [(8 * i, 0) for i in range(64)], 64, 0.5)  # exactly at the limit (T * P = 16384): accepted


# ---- the wrapper around a stub model: against the reference's own wrapper (live, and recorded for the GPU leg)
class _Stub(torch.nn.Module):
    """Prepared decoded predictions per tile, handed out in the order the tiles are forwarded (tests/make_sliding_window_golden.py)."""

    def __init__(self, case, device):
        super().__init__()
        self.case, self.device, self.cursor, self.calls = case, device, 0, []

    def forward(self, x):
        i, self.cursor = self.cursor, self.cursor + x.shape[0]
        self.calls.append(int(x.shape[0]))
        return (self.case["boxes"][i:self.cursor].to(self.device), self.case["scores"][i:self.cursor].to(self.device)), None

    def get_dataset_processing_params(self):
        return dict(class_names=None, image_processor=None, iou=None, conf=None, nms_top_k=None, max_predictions=None, multi_label_per_box=None,
                    class_agnostic_nms=None)

    def get_post_prediction_callback(self, *, conf, iou, nms_top_k, max_predictions, multi_label_per_box, class_agnostic_nms):
        from super_gradients_amd.training.models.detection_models.pp_yolo_e.post_prediction_callback import PPYoloEPostPredictionCallback

        return PPYoloEPostPredictionCallback(score_threshold=conf, nms_threshold=iou, nms_top_k=nms_top_k, max_predictions=max_predictions,
                                             multi_label_per_box=multi_label_per_box, class_agnostic_nms=class_agnostic_nms)


def _product_on_case(case, device, class_agnostic, chunk=32):
    stub = _Stub(case, device)
    w = _wrapper_cls()(tile_size=case["tile_size"], tile_step=case["tile_step"], model=stub, min_tile_threshold=case["min_tile_threshold"],
                       tile_nms_iou=case["iou"], tile_nms_conf=case["conf"], tile_nms_top_k=case["nms_top_k"],
                       tile_nms_max_predictions=case["max_predictions"], tile_nms_multi_label_per_box=True, tile_nms_class_agnostic_nms=class_agnostic)
    assert w.max_tiles_per_forward == 32
    w.max_tiles_per_forward = chunk
    res = w(torch.zeros(case["B"], 3, case["H"], case["W"], device=device))
    assert sum(stub.calls) == case["B"] * case["T"] and max(stub.calls) <= chunk
    return res


@pytest.mark.parametrize("class_agnostic", [False, True])
def test_wrapper_around_stub_equals_recorded_reference(backend, class_agnostic):
    """Product wrapper == the rows the reference's own wrapper returned for the same prepared tile predictions (class-agnostic tile stage
    followed by the per-class merge included)."""
    case = torch.load(os.path.join(GOLDEN, "sliding_window_merge.pt"), weights_only=True)
    want = case["expected_class_agnostic_tiles" if class_agnostic else "expected_per_class"]
    for chunk in (32, 5):
        got = _product_on_case(case, backend, class_agnostic, chunk)
        assert len(got) == len(want) == case["B"]
        for g, w in zip(got, want):
            assert g.shape == w.shape and w.shape[0] > 0 and torch.equal(g.cpu().view(torch.int32), w.view(torch.int32))


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
@pytest.mark.parametrize("class_agnostic", [False, True])
def test_wrapper_around_stub_equals_live_reference(class_agnostic):
    import emu_env
    import make_sliding_window_golden as G

    case = torch.load(os.path.join(GOLDEN, "sliding_window_merge.pt"), weights_only=True)
    fresh = G.merge_case_inputs()
    assert torch.equal(fresh["boxes"], case["boxes"]) and torch.equal(fresh["scores"], case["scores"])
    ref = G.run_reference(G.reference_wrapper_class(), case, class_agnostic)
    rec = case["expected_class_agnostic_tiles" if class_agnostic else "expected_per_class"]
    emu_env.activate()
    try:
        got = _product_on_case(case, torch.device("cpu"), class_agnostic)
    finally:
        emu_env.deactivate()
    n_tile_rows = 0
    for r, g, w in zip(ref, got, rec):
        assert torch.equal(r, w) and torch.equal(g, r)
        n_tile_rows += len(r)
    assert n_tile_rows > 0


def test_wrapper_refuses_what_has_no_device_path(backend):
    case = torch.load(os.path.join(GOLDEN, "sliding_window_merge.pt"), weights_only=True)
    w = _wrapper_cls()(tile_size=64, tile_step=48, model=_Stub(case, backend))
    with pytest.raises(NotImplementedError, match="forward_batched"):
        w(torch.zeros(1, 3, 150, 180, device=backend), sliding_window_post_prediction_callback=lambda out: out)
    with pytest.raises(NotImplementedError, match="cv2"):
        w.predict_webcam()
    w.set_dataset_processing_params(max_predictions=300)
    w.tile_step = 4  # 23 x 30 tiles x 300 rows: past the merge kernel's capacity
    with pytest.raises(ValueError, match="merged rows"):
        w(torch.zeros(1, 3, 150, 180, device=backend))


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. real models
def _detector(name, device):
    from super_gradients_amd.training import models
    from test_predict import _shrunk_arch

    torch.manual_seed(21)
    if name == "yolo_nas_s":
        net = models.get("yolo_nas_s", num_classes=3, arch_params=None if device.type == "cuda" else _shrunk_arch())
    else:
        net = models.get("ppyoloe_s", num_classes=3)
    g = torch.Generator().manual_seed(11)
    for m in net.modules():
        if hasattr(m, "running_var"):
            m.running_mean.normal_(0, 0.1, generator=g)
            m.running_var.uniform_(0.8, 1.2, generator=g)
    net.materialize(device)
    return net.eval()


@pytest.mark.parametrize("name", ["yolo_nas_s", "ppyoloe_s"])
def test_wrapper_wiring_and_batched_tiles(backend, name):
    """wrapper.forward == oracle merge o callback.forward o model on the same gathered tile chunks (one chunk, and max_tiles_per_forward <
    B * T); and the decoded boxes / scores of the tile batch against every tile forwarded alone, before NMS, at the 1e-4 activation bar."""
    from super_gradients_amd import kernels as K

    net = _detector(name, backend)
    tile, step = 64, 32
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 96, 128, generator=g).to(backend)
    w = _wrapper_cls()(tile_size=tile, tile_step=step, model=net, tile_nms_conf=0.0, tile_nms_iou=0.6, tile_nms_top_k=200, tile_nms_max_predictions=30)
    cb = w.sliding_window_post_prediction_callback
    origins, _, _ = w._tile_grid(96, 128)
    T = len(origins)
    assert T >= 6 and step < tile
    tiles, _ = w._gather(x)
    with torch.no_grad():
        for chunk in (32, 5):
            assert (chunk < 2 * T) == (chunk == 5)
            w.max_tiles_per_forward = chunk
            got = w(x)
            tile_rows = []
            for s in range(0, 2 * T, chunk):
                tile_rows += [r.cpu() for r in cb.forward(net(K.nhwc_as_nchw_view(tiles[s:s + chunk], 3)))]
            assert sum(len(r) > 0 for r in tile_rows) > T  # most tiles contribute rows
            want = oracle_merge(tile_rows, origins, T, 0.6)
            for a, b in zip(got, want):
                assert a.shape == b.shape and len(b) > 0 and torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))
        boxes, scores = net(K.nhwc_as_nchw_view(tiles, 3))[0]
        for i in range(2 * T):
            b1, s1 = net(K.nhwc_as_nchw_view(tiles[i:i + 1], 3))[0]
            eb, es = rel_err(boxes[i:i + 1].cpu(), b1.cpu()), rel_err(scores[i:i + 1].cpu(), s1.cpu())
            print(f"{name} tile {i}: batched vs alone rel err boxes {eb:.2e} scores {es:.2e}")
            assert eb < 1e-4 and es < 1e-4


# ---------------------------------------------------------------------------------------------------------------- 6. predict()
def _predict_setup(backend):
    from super_gradients_amd.training.processing import ComposeProcessing, DetectionLongestMaxSizeRescale, DetectionCenterPadding, ImagePermute, StandardizeImage
    from test_predict import _small_detector

    net = _small_detector(backend)
    net.set_dataset_processing_params(class_names=["a", "b", "c"], iou=0.6, conf=0.0, image_processor=ComposeProcessing(
        [DetectionLongestMaxSizeRescale((62, 62)), DetectionCenterPadding((64, 64), 114), StandardizeImage(255.0), ImagePermute()]))
    rng = np.random.default_rng(9)
    sizes = [(100, 130, 3), (100, 130, 3), (150, 97, 3)]
    return net, [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]


@pytest.mark.parametrize("fp16", [False, True])
def test_predict_end_to_end(backend, fp16):
    """predict() of the wrapper on raw uint8 images larger than the tile (two sizes, skip_image_resizing=True): result types, per-image
    counts and boxes equal the wrapper-level result of the pipeline's own fused model on the pre-processed batch, mapped back on the host by
    the processing stages' postprocess_predictions; predict() of the plain model is unchanged by constructing / using a wrapper."""
    import warnings

    from super_gradients_amd.training.pipelines import SlidingWindowDetectionPipeline
    from super_gradients_amd.training.utils.predict import DetectionPrediction, ImageDetectionPrediction, ImagesDetectionPrediction

    net, images = _predict_setup(backend)
    kw = dict(conf=0.0, iou=0.6, nms_top_k=100, max_predictions=20, fp16=fp16, skip_image_resizing=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        before = net.predict(images[:2], **kw)
        w = _wrapper_cls()(tile_size=64, tile_step=48, model=net)
        assert w.get_processing_params() is net.get_processing_params() and w.get_input_channels() == 3
        res = w.predict(images[:2], **kw)
        one = w.predict(images[2], **kw)
        after = net.predict(images[:2], **kw)
    for a, b in zip(before, after):
        assert np.array_equal(a.prediction.bboxes_xyxy, b.prediction.bboxes_xyxy) and np.array_equal(a.prediction.confidence, b.prediction.confidence)
        assert np.array_equal(a.prediction.labels, b.prediction.labels)
    assert isinstance(res, ImagesDetectionPrediction) and len(res) == 2 and isinstance(one, ImageDetectionPrediction)
    pipe = w._get_pipeline(**kw)
    assert isinstance(pipe, SlidingWindowDetectionPipeline) and pipe is w._get_pipeline(**kw)
    assert pipe.model is not w and pipe.model.model is not net and pipe.half == (fp16 and net.supports_half_inference())
    for group, got_group in (((images[0], images[1]), list(res)), ((images[2],), [one])):
        batch, metas = pipe.image_processor.preprocess_batch(list(group), device=backend)
        assert batch.shape[-2] % 32 == 0 and batch.shape[-1] % 32 == 0 and batch.shape[-2] > 64 and batch.shape[-1] > 64
        rows = pipe.model(batch, sliding_window_post_prediction_callback=pipe.post_prediction_callback)
        for img, r, md, got in zip(group, rows, metas, got_group):
            r = r.cpu().numpy()
            host = pipe.image_processor.postprocess_predictions(
                DetectionPrediction(bboxes=r[:, :4], confidence=r[:, 4], labels=r[:, 5].astype(int), bbox_format="xyxy", image_shape=tuple(batch.shape[1:])), md)
            assert got.image is img and len(got.prediction) == len(r) > 0
            assert np.array_equal(got.prediction.bboxes_xyxy, host.bboxes_xyxy) and np.array_equal(got.prediction.confidence, r[:, 4])
            assert np.array_equal(got.prediction.labels, r[:, 5].astype(int))


def _confined_detector(device):
    """test_predict's small seeded detector with +8 on the first bin of every distance distribution (the reg_pred biases): every decoded
    side lies well under half a stride from its anchor point, so a tile's boxes lie inside the tile - what a trained detector's boxes do
    for objects inside the tile.  With the default bias an untrained head decodes near-uniform distributions, about 8 strides to every
    side, and boxes leave the image whatever the tiled path does (neither the reference nor this package clips boxes)."""
    from super_gradients_amd.training import models
    from test_predict import _shrunk_arch

    net = models.get("yolo_nas_s", num_classes=3, arch_params=None if device.type == "cuda" else _shrunk_arch())
    g = torch.Generator().manual_seed(11)
    for m in net.modules():
        if hasattr(m, "running_var"):
            m.running_mean.normal_(0, 0.1, generator=g)
            m.running_var.uniform_(0.8, 1.2, generator=g)
    for head in net.heads.heads if hasattr(net.heads, "heads") else [m for m in net.heads.modules() if hasattr(m, "reg_pred")]:
        with torch.no_grad():
            head.reg_pred.bias.view(4, -1)[:, 0] += 8.0
    net.materialize(device)
    return net


@pytest.mark.parametrize("fp16", [False, True])
def test_predict_boxes_lie_inside_the_image(backend, fp16):
    """Boxes of predict() must lie inside the original image extent: raw uint8 images larger than the tile in two sizes, skip_image_resizing.
    The detector's own boxes lie inside their tile (_confined_detector; asserted first on one gathered tile batch), and the image sizes
    are ones whose tiles cover exactly the image (160 x 160: exact fit; 112 x 160: padded to 128 rows, the 16-row remainder is under
    min_tile_threshold and dropped) - so a box outside the image can only come from the tile shifts, the merge or the inverse maps."""
    import warnings

    from super_gradients_amd import kernels as K
    from super_gradients_amd.training.processing import ComposeProcessing, DetectionCenterPadding, DetectionLongestMaxSizeRescale, ImagePermute, StandardizeImage

    net = _confined_detector(backend)
    net.set_dataset_processing_params(class_names=["a", "b", "c"], iou=0.6, conf=0.0, image_processor=ComposeProcessing(
        [DetectionLongestMaxSizeRescale((62, 62)), DetectionCenterPadding((64, 64), 114), StandardizeImage(255.0), ImagePermute()]))
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(160, 160, 3), (160, 160, 3), (112, 160, 3)]]
    w = _wrapper_cls()(tile_size=64, tile_step=48, model=net)
    kw = dict(conf=0.0, iou=0.6, nms_top_k=100, max_predictions=20, fp16=fp16, skip_image_resizing=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        preds = list(w.predict(images[:2], **kw)) + [w.predict(images[2], **kw)]
        pipe = w._get_pipeline(**kw)
    batch, _ = pipe.image_processor.preprocess_batch(images[:2], device=backend)
    tiles, origins = pipe.model._gather(batch)
    assert len(origins) == 9
    with torch.no_grad():
        tb = pipe.model.model(K.nhwc_as_nchw_view(tiles, 3))[0][0].cpu()
    print(f"fp16={fp16} tile boxes in [{float(tb.min()):.2f}, {float(tb.max()):.2f}]")
    assert float(tb.min()) >= 0 and float(tb.max()) <= 64
    for img, p in zip(images, preds):
        b = p.prediction.bboxes_xyxy
        h, wd = img.shape[:2]
        print(f"fp16={fp16} image {wd}x{h}: {len(b)} boxes, x in [{b[:, [0, 2]].min():.2f}, {b[:, [0, 2]].max():.2f}], y in [{b[:, [1, 3]].min():.2f}, {b[:, [1, 3]].max():.2f}]")
        assert len(b) > 0 and b[:, [0, 2]].min() >= 0 and b[:, [0, 2]].max() <= wd and b[:, [1, 3]].min() >= 0 and b[:, [1, 3]].max() <= h
        assert b[:, [0, 2]].max() > wd / 2 and b[:, [1, 3]].max() > h / 2  # (detections do come from the far tiles)
