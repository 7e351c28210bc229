"""The three consumers of the model's raw output behind the rotated NMS (dpft_amd/evaluation/nms.py): a query that was taken out
reads as background to the K-Radar exporter, to DatasetAP and to the evaluation loop, none of which changed.  References: the
fp64 restatements tests/nms_ref.py and tests/dataset_ap_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dataset_ap_ref as G
from tests import nms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
C4 = 4
NMS = dict(iou=0.3, kind="bev", class_agnostic=False)
AP = dict(G.K6, recall_points=40)
THRS = [0.0, 0.9, 1.6]


@functools.lru_cache(maxsize=None)
def _case():
    """3 frames of 65 queries with ground truth (dataset_ap_ref's sample builder: half the queries are perturbed copies of targets
    inside the exporter's field of view, so they crowd), redrawn until the NMS reference AND the AP reference on the kept subset
    are safe to compare exactly.  Returns (samples, NMS reference, samples with the non-kept queries made background)."""
    for attempt in range(100):
        rng = np.random.default_rng(777 + attempt)
        samples = [G.random_sample(rng, 65, m, C4) for m in (9, 0, 5)]
        frames = [{k: s[k] for k in ("cls", "center", "size", "angle")} for s in samples]
        if R.violations(frames, **NMS):
            continue
        ref = R.run(frames, **NMS)
        kept = []
        for s, st in zip(samples, ref["status"]):
            k = {key: v.copy() for key, v in s.items()}
            gone = (st >= 0) | (st == R.BELOW_MIN_SCORE) | (st == R.BEYOND_MAX_DET)
            k["cls"][gone] = np.float32(0.0)
            k["cls"][gone, 0] = np.float32(1.0)                       # the kept subset: everything else is plain background
            kept.append(k)
        if G.violations([(20 + b, k) for b, k in enumerate(kept)], C4, AP):
            continue
        assert sum(int((st >= 0).sum()) for st in ref["status"]) >= 10
        return samples, ref, kept
    raise AssertionError("no safe draw in 100 attempts")


def _output(samples):
    return {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(DEV)
            for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}


def _labels(samples):
    return [dict({k: torch.from_numpy(s[k]).to(DEV) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")},
                 description=torch.tensor([b % 8, b % 2, b % 7], device=DEV)) for b, s in enumerate(samples)]


def _nms():
    from dpft_amd.evaluation.nms import RotatedNMS
    return RotatedNMS(**NMS)


def _expected_rows(output, status):
    """``select`` on the raw output with the rows of the non-kept queries removed: per (sample, threshold) the surviving rows."""
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    rows, counts, mask = (t.cpu().numpy() for t in KRadarExporter.select(output["class"], output["center"], output["size"],
                                                                        output["angle"], THRS))
    out = []
    for b in range(rows.shape[0]):
        per_thr = []
        for t in range(len(THRS)):
            queries = np.nonzero((mask[b] >> t) & 1)[0]                # candidate order = query order
            assert len(queries) == counts[b, t]
            per_thr.append(rows[b, t, :counts[b, t]][status[b][queries] == R.KEPT])
        out.append(per_thr)
    return out


def test_exporter_select_on_the_suppressed_output_is_select_without_the_removed_queries():
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    samples, ref, _ = _case()
    out = _output(samples)
    want = _expected_rows(out, ref["status"])
    sup = _nms().suppress(out)
    rows, counts, _mask = (t.cpu().numpy() for t in KRadarExporter.select(sup["class"], sup["center"], sup["size"], sup["angle"], THRS))
    removed = 0
    for b in range(len(samples)):
        for t in range(len(THRS)):
            assert counts[b, t] == len(want[b][t]), (b, t, counts[b, t], len(want[b][t]))
            assert np.array_equal(rows[b, t, :counts[b, t]].view(np.uint32), want[b][t].view(np.uint32))
    raw = KRadarExporter.select(out["class"], out["center"], out["size"], out["angle"], THRS)[1].cpu().numpy()
    removed = int(raw.sum() - counts.sum())
    print("rows removed from the export:", removed)
    assert removed > 0


def _records(ap):
    rec = ap.state()["records"].cpu().numpy()
    score = rec[:, 0].copy().view(np.float32).astype(np.float64)
    cols = np.stack([rec[:, 0], rec[:, 1], rec[:, 2] & 0xFFFF, (rec[:, 2] >> 16) & 0xFF, rec[:, 3]], 1).astype(np.int64)
    return cols[np.lexsort((cols[:, 2], cols[:, 1], -score, cols[:, 3]))]


def test_dataset_ap_on_the_suppressed_output_is_the_reference_on_the_kept_subset():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    samples, _ref, kept = _case()
    want = G.run([(20 + b, k) for b, k in enumerate(kept)], C4, **AP)
    raw = G.run([(20 + b, s) for b, s in enumerate(samples)], C4, **AP)
    assert want["records"].shape[0] < raw["records"].shape[0]
    ap = DatasetAP(C4, **AP)
    ap.update(_nms().suppress(_output(samples)), _labels(samples), 20)
    got = _records(ap)
    assert got.shape == want["records"].shape and np.array_equal(got, want["records"])
    res = ap.compute()
    assert np.array_equal(res["npos"].numpy(), want["npos"]) and np.array_equal(res["tp"].numpy(), want["tp"])
    err = np.nanmax(np.abs(res["ap"].numpy() - want["ap"]), initial=0.0)
    print("max |ap - ref| =", err)
    assert err <= 1e-12 and np.array_equal(np.isnan(res["ap"].numpy()), np.isnan(want["ap"]))      # (test_gpu_dataset_ap's bound)


def test_detections_rows_equal_the_reference():
    samples, ref, _ = _case()
    frames = [{k: s[k] for k in ("cls", "center", "size", "angle")} for s in samples]
    want = R.detections(frames, ref)
    got = _nms().detections(_output(samples))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == w.shape and w.shape[1] == 10
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))


class _FixedModel(torch.nn.Module):
    """Returns the prepared output dicts one batch after the other."""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls = outputs, 0

    def forward(self, data):
        self.calls += 1
        return self.outputs[self.calls - 1]


def test_evaluator_hands_the_suppressed_dict_to_metric_dataset_ap_and_exporter(tmp_path):
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    samples, ref, kept = _case()
    batches = [samples[:2], samples[2:]]
    outputs = [_output(b) for b in batches]
    loader = [({"x": torch.zeros(len(b), 1)}, _labels(b)) for b in batches]
    seen = {"metric": [], "ap": [], "export": []}

    def metric(output, labels):
        seen["metric"].append(output)
        return {"n": torch.tensor(float(len(labels)), device=DEV)}

    class RecordingAP(DatasetAP):
        def update(self, output, labels, first_frame):
            seen["ap"].append(output)
            return super().update(output, labels, first_frame)

    exporter = KRadarExporter(conf_thrs=THRS)

    def export(output, labels, step, dst):
        seen["export"].append(output)
        return exporter(output, labels, step, dst)

    ev = DataParallelEvaluator(metric=metric, exporter=export, device=DEV, dataset_ap=RecordingAP(C4, **AP), nms=_nms())
    model = _FixedModel(outputs)
    scalars = ev.evaluate_one_epoch(0, model, loader, dst=str(tmp_path), shard_start=20)
    assert model.calls == 2 and [len(v) for v in seen.values()] == [2, 2, 2]
    b0 = 0
    for i, raw in enumerate(outputs):
        got = seen["metric"][i]
        assert got is seen["ap"][i] and got is seen["export"][i] and got is not raw and list(got) == list(raw)
        assert all(got[k] is raw[k] for k in raw if k != "class")
        n = raw["class"].shape[0]
        assert np.array_equal(got["class"].cpu().numpy().view(np.uint32), ref["cls_out"][b0:b0 + n].view(np.uint32))
        b0 += n
    want = G.run([(20 + b, k) for b, k in enumerate(kept)], C4, **AP)
    assert scalars["mAP_bev@0.3"] == pytest.approx(want["mAP"][0], abs=1e-12) and scalars["n"] == 1.5
    # the exported prediction files hold the kept boxes only
    rows = _expected_rows(_output(samples), ref["status"])
    for b in range(len(samples)):
        for t, thr in enumerate(THRS):
            path = os.path.join(str(tmp_path), "exports", "kradar", str(thr), "all", "preds", f"{20 + b:06d}.txt")
            lines = open(path).read().splitlines()
            assert lines == (exporter._serialize_rows(rows[b][t]) or exporter._get_dummy_object()), (b, thr)
    n_lines = sum(len(rows[b][0]) for b in range(len(samples)))
    print("exported boxes at threshold 0:", n_lines)
    assert n_lines > 0


def test_evaluator_without_nms_hands_the_raw_dict_on():
    from dpft_amd.evaluation import DataParallelEvaluator
    samples, _, _ = _case()
    out = _output(samples)
    seen = []
    ev = DataParallelEvaluator(metric=lambda o, l: seen.append(o) or {}, device=DEV)
    ev.evaluate_one_epoch(0, _FixedModel([out]), [({"x": torch.zeros(3, 1)}, _labels(samples))])
    assert seen[0] is out and ev.nms is None
