from .pipelines import DetectionPipeline, Pipeline, SlidingWindowDetectionPipeline  # noqa: F401
