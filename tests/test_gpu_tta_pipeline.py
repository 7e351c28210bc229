"""``DataParallelEvaluator`` with ``evaluate.tta``: every forward of ``evaluate_one_epoch`` becomes T forwards and the fusion, in front
of the NMS; ``Metric``, ``DatasetAP`` and the exporter read the (B, T N) dict.  The small input-driven model, split and loader are
those of tests/test_gpu_robustness.py."""
import math

import numpy as np
import pytest
import torch

from tests import test_gpu_robustness as RB

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUTS = [(0, 4), (4, 6)]
CONDITION = {"conditions": {"noisy": RB.CONDITIONS["noisy"]}, "seed": 5}


def _tta(**kw):
    from dpft_amd.evaluation.tta import TestTimeAugmentation
    return TestTimeAugmentation(**kw)


def _evaluator(tta=None, nms=None, robustness=None, exporter=None, metric=RB._metric):
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    return DataParallelEvaluator(metric=metric, exporter=exporter, device=DEV, dataset_ap=DatasetAP(RB.C4, groups=["weather"], **RB.AP),
                                 nms=nms, robustness=robustness, tta=tta)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_the_same_keys_as_without_the_key_and_finite_values():
    plain = _evaluator().evaluate_one_epoch(0, RB._InputDrivenModel(), RB._loader(CUTS), shard_start=0)
    model = RB._InputDrivenModel()
    ev = _evaluator(tta=_tta())
    scalars = ev.evaluate_one_epoch(0, model, RB._loader(CUTS), shard_start=0)
    assert model.calls == 2 * 2 and set(scalars) == set(plain) and scalars
    for k, v in scalars.items():
        assert math.isnan(v) == math.isnan(plain[k]), k              # (NaN: a class without ground truth in a group)
        assert math.isnan(v) or math.isfinite(v), k
    # the second forward of a batch saw the mirrored views
    for k in ("camera_mono", "radar_bev", "radar_front"):
        assert torch.equal(model.seen[1][k], model.seen[0][k].flip(2)) and not torch.equal(model.seen[1][k], model.seen[0][k])


def test_everything_switched_on_together_and_the_consumers_read_the_fused_dict():
    from dpft_amd.evaluation.nms import RotatedNMS
    from dpft_amd.evaluation.robustness import RobustnessSuite
    seen = {"metric": [], "export": []}

    def metric(output, labels):
        seen["metric"].append(output)
        return RB._metric(output, labels)

    tta, nms = _tta(views=[{"flip": True}, {"zoom": 1.1}], score="max"), RotatedNMS(iou=0.2)
    ev = _evaluator(tta=tta, nms=nms, robustness=RobustnessSuite(CONDITION), metric=metric,
                    exporter=lambda output, labels, step, dst: seen["export"].append((output, step)))
    from dpft_amd.evaluation.dataset_ap import DatasetAP

    class RecordingAP(DatasetAP):                                     # (a condition's accumulator is a deep copy: its own log)
        def update(self, output, labels, first_frame):
            self.log.append(output)
            return super().update(output, labels, first_frame)

    ev.dataset_ap = RecordingAP(RB.C4, groups=["weather"], **RB.AP)
    ev.dataset_ap.log = seen["ap"] = []
    model = RB._InputDrivenModel()
    scalars = ev.evaluate_one_epoch(0, model, RB._loader(CUTS), dst="unused", shard_start=0)
    T, M = 3, 3 * RB.NQ
    assert model.calls == 2 * 2 * T and "score/cond=noisy" in scalars and "mAP_3d@0.5/cond=noisy" in scalars
    assert [step for _, step in seen["export"]] == [0, 4] and len(seen["ap"]) == 2 and len(seen["metric"]) == 4
    for j, (a, b) in enumerate(CUTS):
        outs = model.outputs[2 * T * j: 2 * T * j + T]                # the clean forwards of batch j
        want = nms.suppress(tta.fuse(outs))
        got = seen["export"][j][0]
        assert got is seen["ap"][j] and got is seen["metric"][2 * j]
        assert list(got) == list(outs[0])
        for k in want:
            assert tuple(got[k].shape)[:2] == (b - a, M) and _bits_equal(got[k], want[k]), k
        noisy = nms.suppress(tta.fuse(model.outputs[2 * T * j + T: 2 * T * (j + 1)]))
        assert all(_bits_equal(seen["metric"][2 * j + 1][k], noisy[k]) for k in noisy)
        # the zoomed view kept the radar maps, the flipped one mirrored the degraded ones
        s = model.seen[2 * T * j + T:]
        assert s[2]["radar_bev"] is s[0]["radar_bev"] and torch.equal(s[1]["radar_bev"], s[0]["radar_bev"].flip(2))


class _Prepared:
    """Returns prepared outputs one after the other."""

    def __init__(self, outputs):
        self.outputs, self.calls = outputs, 0

    def __call__(self, data):
        self.calls += 1
        return self.outputs[self.calls - 1]


def test_exact_mirrors_fuse_to_the_score_and_the_centre_of_view_0():
    rng = np.random.default_rng(11)
    N, C = 33, 3
    cls = rng.normal(-2, 0.2, (2, N, C)).astype(np.float32)
    score = rng.permutation(np.linspace(0.1, 3.0, 2 * N)).astype(np.float32).reshape(2, N)
    cls[:, :, 1] = score
    center = np.stack([np.tile(6.0 * np.arange(N, dtype=np.float32), (2, 1)), rng.uniform(-40, 40, (2, N)), rng.uniform(-1, 1, (2, N))],
                      -1).astype(np.float32)
    size = rng.uniform(1.0, 4.0, (2, N, 3)).astype(np.float32)
    yaw = rng.uniform(-math.pi, math.pi, (2, N))
    angle = np.stack([np.sin(yaw), np.cos(yaw)], -1).astype(np.float32)
    v0 = {k: torch.from_numpy(v).to(DEV) for k, v in (("class", cls), ("center", center), ("size", size), ("angle", angle))}
    v1 = {k: v.clone() for k, v in v0.items()}
    v1["center"][:, :, 1] = -v1["center"][:, :, 1]
    v1["angle"][:, :, 0] = -v1["angle"][:, :, 0]
    tta = _tta(score="mean")
    model = _Prepared([v0, v1])
    fused = tta(model, {"frame": torch.arange(2, device=DEV)})
    status, order, counts, members = tta.clusters([v0, v1])
    assert model.calls == 2 and counts.tolist() == [N, N]
    assert bool((members[:, :N] == 2).all()) and bool((members[:, N:] == 0).all())
    assert bool((status[:, :N] == -1).all()) and torch.equal(status[:, N:].cpu(), torch.arange(N, dtype=torch.int32).expand(2, N))
    want = ((score.astype(np.float64) + score.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(fused["class"][:, :N, 1].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((fused["class"][:, :N, 0] == 0).all()) and bool((fused["class"][:, :N, 2] == 0).all())
    got = fused["center"][:, :N].cpu().numpy()
    ulp = np.spacing(np.abs(center))
    assert np.all(np.abs(got.astype(np.float64) - center.astype(np.float64)) <= ulp)
    # the members read as background and keep the mirrored-back geometry bits of view 1 (= view 0's)
    assert _bits_equal(fused["center"][:, N:], v0["center"]) and bool((fused["class"][:, N:, 0] == v0["class"][:, :, 1]).all())


def test_without_the_key_the_outputs_keep_their_bits():
    model = RB._InputDrivenModel()
    ev = _evaluator()
    assert ev.tta is None
    exported = []
    ev.export_fn = lambda output, labels, step, dst: exported.append(output)
    scalars = ev.evaluate_one_epoch(0, model, RB._loader(CUTS), dst="unused", shard_start=0)
    assert model.calls == 2 and all(o is m for o, m in zip(exported, model.outputs))      # the model's own dicts, no launch between
    other = RB._evaluator(robustness=False).evaluate_one_epoch(0, RB._InputDrivenModel(), RB._loader(CUTS), shard_start=0)
    assert set(other) == set(scalars)
    for k, v in other.items():
        assert RB._same(v, scalars[k]), k
