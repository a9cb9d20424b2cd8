"""Inference engine: graph-replayed scoring of window loaders (:class:`Predictor`)."""
from .predictor import Predictor, predict_emit, series_tm_gather

__all__ = ["Predictor", "predict_emit", "series_tm_gather"]
