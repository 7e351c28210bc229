"""Evaluation-side pieces: the per-step metrics, the split-level AP (dataset_ap.py), the optional rotated NMS (nms.py), and the K-Radar exporter."""
from dpft_amd.evaluation.metric import Metric, build_metric   # noqa: F401
from dpft_amd.evaluation.evaluator import DataParallelEvaluator, build_evaluator, merge_rank_exports   # noqa: F401
from dpft_amd.evaluation.dataset_ap import DatasetAP   # noqa: F401
from dpft_amd.evaluation.nms import RotatedNMS   # noqa: F401
