"""SlidingWindowInferenceDetectionWrapper on the HIP kernels: a detector trained on tile_size x tile_size inputs run over a larger image.

Reference: training/models/detection_models/sliding_window_detection_forward_wrapper.py:18-392 - same constructor, forward signature and
result (a list of B tensors [Ni, 6] = x1, y1, x2, y2, confidence, class in the frame of the input image; an image without detections gives
an empty [0, 6] tensor), same processing-parameter and predict() surface.  What differs is where the work runs:

  reference (forward :100-134)                                  here
  Python loop over images, then over tiles                      the tile grid is computed once on the host (the reference's arithmetic, :136-156)
  one slice of a zero-padded copy per tile                      ONE launch cuts every tile of the batch (kernels.tile_gather, csrc/image.hip)
  one batch-1 forward per tile                                  the B*T tiles go through the model in chunks of max_tiles_per_forward
  one post-prediction callback call per tile                    the callback's batched form on every chunk (csrc/nms.hip, no host round trip)
  one small host-built offset tensor per tile, torch.cat and    ONE cross-tile merge for the batch (kernels.tile_merge, csrc/nms.hip): the shift
  torchvision.ops.batched_nms per image                         by the tile origin and torchvision's CPU batched_nms arithmetic, on the device
The only host synchronisation of forward() is the final read of the B merged counts; forward_batched() has none.
"""
from typing import List, Optional, Tuple

import torch
from torch import nn

from .... import kernels as K


class SlidingWindowInferenceDetectionWrapper(nn.Module):
    def __init__(self, tile_size: int, tile_step: int, model, min_tile_threshold: int = 30, tile_nms_iou: Optional[float] = None,
                 tile_nms_conf: Optional[float] = None, tile_nms_top_k: Optional[int] = None, tile_nms_max_predictions: Optional[int] = None,
                 tile_nms_multi_label_per_box: Optional[bool] = None, tile_nms_class_agnostic_nms: Optional[bool] = None):
        super().__init__()
        if int(tile_size) <= 0 or int(tile_step) <= 0:
            raise ValueError(f"tile_size and tile_step must be positive (got {tile_size}, {tile_step})")
        self.tile_size, self.tile_step, self.min_tile_threshold = tile_size, tile_step, min_tile_threshold
        # tiles per model forward (not in the reference, which forwards one tile at a time): 32 is the batch the conv tuning tables are made for
        self.max_tiles_per_forward = 32

        self._class_names: Optional[List[str]] = None
        self._image_processor = None
        self._default_nms_iou, self._default_nms_conf, self._default_nms_top_k = 0.7, 0.5, 1024
        self._default_max_predictions, self._default_multi_label_per_box, self._default_class_agnostic_nms = 300, True, False
        self._pipeline_cache = None
        self._origins_cache = {}

        self.model = model
        self.set_dataset_processing_params(**self.model.get_dataset_processing_params())  # :74 (the tile thresholds start from the model's)
        if any(a is not None for a in (tile_nms_iou, tile_nms_conf, tile_nms_top_k, tile_nms_max_predictions, tile_nms_multi_label_per_box,
                                       tile_nms_class_agnostic_nms)):
            self.set_dataset_processing_params(iou=tile_nms_iou, conf=tile_nms_conf, nms_top_k=tile_nms_top_k, max_predictions=tile_nms_max_predictions,
                                               multi_label_per_box=tile_nms_multi_label_per_box, class_agnostic_nms=tile_nms_class_agnostic_nms)
        else:  # :89-98
            self.sliding_window_post_prediction_callback = self.get_post_prediction_callback(
                iou=self._default_nms_iou, conf=self._default_nms_conf, nms_top_k=self._default_nms_top_k, max_predictions=self._default_max_predictions,
                multi_label_per_box=self._default_multi_label_per_box, class_agnostic_nms=self._default_class_agnostic_nms)

    # ---- the tile grid (host) ------------------------------------------------------------------------------------------------------
    def _tile_grid(self, h: int, w: int) -> Tuple[List[Tuple[int, int]], int, int]:
        """_generate_tiles (:136-156) without the pixels: the (x, y) origins in the reference's order (rows of tiles, left to right) and the
        extent (max_y, max_x) the reference pads the image to.  Python's modulo: an image smaller than a tile has a negative h - tile_size,
        and the reference then pads it up to a multiple - mirrored, not "fixed"."""
        ts, step, thr = self.tile_size, self.tile_step, self.min_tile_threshold
        max_y = h if (h - ts) % step < thr else h - (h - ts) % step + ts
        max_x = w if (w - ts) % step < thr else w - (w - ts) % step + ts
        origins = [(x, y) for y in range(0, max_y - ts + 1, step) for x in range(0, max_x - ts + 1, step)]
        return origins, max(max_y, h), max(max_x, w)

    def _generate_tiles(self, image, tile_size=None, tile_step=None):
        """The reference's method (:136-156): [(tile [N, C, tile, tile], (x, y)), ...] of an NCHW batch - cut by the device gather."""
        if (tile_size, tile_step) not in ((None, None), (self.tile_size, self.tile_step)):
            raise ValueError("_generate_tiles: the grid is the wrapper's own tile_size / tile_step")
        n, c = image.shape[:2]
        tiles, origins = self._gather(image)
        T = len(origins)
        return [(K.nhwc_as_nchw_view(tiles[t::T], c), xy) for t, xy in enumerate(origins)] if T else []

    def _gather(self, inputs):
        """NCHW batch -> (tiles NHWC [B*T, tile, tile, Cpad] fp32, tile t of image b at b*T + t; origins)."""
        origins, _, _ = self._tile_grid(int(inputs.shape[2]), int(inputs.shape[3]))
        if not origins:
            return None, origins
        key = (tuple(origins), inputs.device)
        table = self._origins_cache.get(key)
        if table is None:
            self._origins_cache.clear()
            table = self._origins_cache[key] = torch.tensor(origins, dtype=torch.int32).reshape(-1, 2).to(inputs.device)
        xh = K.input_to_nhwc(inputs).contiguous()
        return K.tile_gather(xh, table, self.tile_size), origins

    # ---- forward -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_batched(self, inputs: torch.Tensor, sliding_window_post_prediction_callback=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-resident result without any host synchronisation: (rows [B, T * P, 6], counts [B] int32), P = the tile stage's
        max_predictions; image b's detections are rows[b, :counts[b]]."""
        cb = sliding_window_post_prediction_callback or self.sliding_window_post_prediction_callback
        if not hasattr(cb, "forward_batched"):
            raise NotImplementedError(f"{type(cb).__name__} has no forward_batched: sliding-window inference runs the tile stage on the device "
                                      "(PPYoloEPostPredictionCallback does); there is no per-tile host path")
        if inputs.dim() != 4:
            raise ValueError(f"expected an NCHW batch, got {tuple(inputs.shape)}")
        if hasattr(self.model, "get_input_shape_steps"):
            (sh, sw), (mh, mw) = self.model.get_input_shape_steps(), self.model.get_minimum_input_shape_size()
            if self.tile_size % sh or self.tile_size % sw or self.tile_size < max(mh, mw):
                raise ValueError(f"tile_size {self.tile_size}: the model takes sizes that are multiples of ({sh}, {sw}) and at least ({mh}, {mw})")
        B, C = int(inputs.shape[0]), int(inputs.shape[1])
        tiles, origins = self._gather(inputs)
        T = len(origins)
        if T == 0:
            raise ValueError(f"a {tuple(inputs.shape[2:])} input has no tile of size {self.tile_size} (step {self.tile_step}, min_tile_threshold "
                             f"{self.min_tile_threshold})")
        P = int(cb.max_predictions)
        if T * P > K.TILE_MERGE_MAX_ROWS:
            raise ValueError(f"{T} tiles x {P} predictions per tile = {T * P} merged rows per image; the merge kernel takes {K.TILE_MERGE_MAX_ROWS} "
                             "(lower tile_nms_max_predictions or raise tile_step)")
        chunk = max(int(self.max_tiles_per_forward), 1)
        rows, counts = [], []
        was_training = self.model.training
        if was_training:
            self.model.eval()
        try:
            for s in range(0, B * T, chunk):
                r, c, _ = cb.forward_batched(self.model(K.nhwc_as_nchw_view(tiles[s:s + chunk], C)))
                rows.append(r)
                counts.append(c)
        finally:
            if was_training:
                self.model.train(True)
        rows = rows[0] if len(rows) == 1 else torch.cat(rows)
        counts = counts[0] if len(counts) == 1 else torch.cat(counts)
        table = self._origins_cache[(tuple(origins), inputs.device)]
        return K.tile_merge(rows, counts, table, T, cb.nms_threshold)  # :127: always per class, the callback's IoU threshold

    def forward(self, inputs: torch.Tensor, sliding_window_post_prediction_callback=None) -> List[torch.Tensor]:
        out, cnt = self.forward_batched(inputs, sliding_window_post_prediction_callback)
        return [out[b, :n] for b, n in enumerate(cnt.tolist())]  # the one host synchronisation

    # ---- processing parameters and predict() (:158-392) ----------------------------------------------------------------------------------
    def get_post_prediction_callback(self, *, conf: float, iou: float, nms_top_k: int, max_predictions: int, multi_label_per_box: bool,
                                     class_agnostic_nms: bool):
        return self.model.get_post_prediction_callback(conf=conf, iou=iou, nms_top_k=nms_top_k, max_predictions=max_predictions,
                                                       multi_label_per_box=multi_label_per_box, class_agnostic_nms=class_agnostic_nms)

    def set_dataset_processing_params(self, class_names: Optional[List[str]] = None, image_processor=None, iou: Optional[float] = None,
                                      conf: Optional[float] = None, nms_top_k: Optional[int] = None, max_predictions: Optional[int] = None,
                                      multi_label_per_box: Optional[bool] = None, class_agnostic_nms: Optional[bool] = None) -> None:
        """:183-233 - unlike the detectors' own method, the thresholds given here do not become defaults of predict(): they rebuild the
        callback forward() uses when it is called without one; a threshold left None takes the general default."""
        from ....common.factories import ProcessingFactory

        if class_names is not None:
            self._class_names = tuple(class_names)
        if image_processor is not None:
            self._image_processor = ProcessingFactory().get(image_processor)  # @resolve_param("image_processor", ProcessingFactory())
        iou = self._default_nms_iou if iou is None else iou
        conf = self._default_nms_conf if conf is None else conf
        nms_top_k = self._default_nms_top_k if nms_top_k is None else nms_top_k
        max_predictions = self._default_max_predictions if max_predictions is None else max_predictions
        multi_label_per_box = self._default_multi_label_per_box if multi_label_per_box is None else multi_label_per_box
        class_agnostic_nms = self._default_class_agnostic_nms if class_agnostic_nms is None else class_agnostic_nms
        self.sliding_window_post_prediction_callback = self.get_post_prediction_callback(
            iou=float(iou), conf=float(conf), nms_top_k=int(nms_top_k), max_predictions=int(max_predictions), multi_label_per_box=bool(multi_label_per_box),
            class_agnostic_nms=bool(class_agnostic_nms))
        self._pipeline_cache = None

    def get_processing_params(self):
        return self._image_processor

    def get_input_channels(self) -> int:
        return self.model.get_input_channels()

    def _around(self, model) -> "SlidingWindowInferenceDetectionWrapper":
        """The same wrapper around another instance of the model (the pipeline's private fused copy)."""
        w = SlidingWindowInferenceDetectionWrapper(self.tile_size, self.tile_step, model, min_tile_threshold=self.min_tile_threshold)
        w.max_tiles_per_forward = self.max_tiles_per_forward
        w._class_names, w._image_processor = self._class_names, self._image_processor
        w.sliding_window_post_prediction_callback = self.sliding_window_post_prediction_callback
        return w

    def _get_pipeline(self, *, iou=None, conf=None, fuse_model: bool = True, skip_image_resizing: bool = False, nms_top_k=None, max_predictions=None,
                      multi_label_per_box=None, class_agnostic_nms=None, fp16: bool = True):
        from ...pipelines.pipelines import SlidingWindowDetectionPipeline
        from ...processing.processing import ComposeProcessing, DetectionAutoPadding

        if None in (self._class_names, self._image_processor, self._default_nms_iou, self._default_nms_conf):
            raise RuntimeError("You must set the dataset processing parameters before calling predict.\n"
                               "Please call `model.set_dataset_processing_params(...)` first or do so on self.model. ")
        key = (iou, conf, fuse_model, skip_image_resizing, nms_top_k, max_predictions, multi_label_per_box, class_agnostic_nms, fp16,
               self.tile_size, self.tile_step, self.min_tile_threshold, self.max_tiles_per_forward)
        if self._pipeline_cache is not None and self._pipeline_cache[0] == key:  # @lru_cache(maxsize=1)
            return self._pipeline_cache[1]
        iou = self._default_nms_iou if iou is None else iou
        conf = self._default_nms_conf if conf is None else conf
        nms_top_k = self._default_nms_top_k if nms_top_k is None else nms_top_k
        max_predictions = self._default_max_predictions if max_predictions is None else max_predictions
        multi_label_per_box = self._default_multi_label_per_box if multi_label_per_box is None else multi_label_per_box
        class_agnostic_nms = self._default_class_agnostic_nms if class_agnostic_nms is None else class_agnostic_nms
        image_processor = self._image_processor
        if isinstance(image_processor, ComposeProcessing) and skip_image_resizing:  # :282-286
            image_processor = image_processor.get_equivalent_compose_without_resizing(DetectionAutoPadding(shape_multiple=(32, 32), pad_value=0))
        pipeline = SlidingWindowDetectionPipeline(
            model=self, image_processor=image_processor, class_names=self._class_names, fuse_model=fuse_model, fp16=fp16,
            post_prediction_callback=self.get_post_prediction_callback(iou=iou, conf=conf, nms_top_k=nms_top_k, max_predictions=max_predictions,
                                                                       multi_label_per_box=multi_label_per_box, class_agnostic_nms=class_agnostic_nms))
        self._pipeline_cache = (key, pipeline)
        return pipeline

    def predict(self, images, iou: Optional[float] = None, conf: Optional[float] = None, batch_size: int = 32, fuse_model: bool = True,
                skip_image_resizing: bool = False, nms_top_k: Optional[int] = None, max_predictions: Optional[int] = None,
                multi_label_per_box: Optional[bool] = None, class_agnostic_nms: Optional[bool] = None, fp16: bool = True):
        """:307-349.  -> ImageDetectionPrediction (one image) / ImagesDetectionPrediction; the thresholds are the tile stage's, the merge uses `iou`."""
        pipeline = self._get_pipeline(iou=iou, conf=conf, fuse_model=fuse_model, skip_image_resizing=skip_image_resizing, nms_top_k=nms_top_k,
                                      max_predictions=max_predictions, multi_label_per_box=multi_label_per_box,
                                      class_agnostic_nms=class_agnostic_nms, fp16=fp16)
        return pipeline(images, batch_size=batch_size)

    def predict_webcam(self, *a, **k):
        raise NotImplementedError("predict_webcam is cv2 camera I/O, outside the MI355X hot path")

    def train(self, mode: bool = True):
        self._pipeline_cache = None  # a cached pipeline holds a fused copy of stale weights (as the detectors' own train())
        return super().train(mode)
