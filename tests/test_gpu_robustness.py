"""``DataParallelEvaluator`` with a ``RobustnessSuite``: after a batch's clean pass every condition runs one more forward on the
degraded batch and feeds its own metric sums and its own split-level AP (``{key}/cond={name}``).  The model here computes its
output from the tensors it receives, so a condition's table shows what reached the model."""
import functools

import numpy as np
import pytest
import torch

from tests import dataset_ap_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
C4, NQ, FRAMES = 4, 33, 6
AP = dict(G.K6, recall_points=40)
CONDITIONS = {"camera_off": {"camera": "off"}, "radar_off": {"radar": "off"},
              "nothing": {"camera": {"haze": 0.0, "blur": 0.0, "noise": 0}, "radar": {"noise": 0.0, "azimuth_mask": []}},
              "fog": {"camera": {"haze": 0.6, "blur": 2.0}},
              "noisy": {"camera": {"noise": 15}, "radar": {"noise": 8}},
              "sector": {"radar": {"azimuth_mask": [[0.4, 0.6]], "range_mask": [[0.0, 0.3]]}}}
SPEC = {"conditions": CONDITIONS, "seed": 5}


@functools.lru_cache(maxsize=None)
def _split():
    """FRAMES frames: prepared queries and targets per frame, camera (12 x 70 x 3) and radar inputs in [0, 255]."""
    rng = np.random.default_rng(4242)
    samples = [G.random_sample(rng, NQ, m, C4) for m in (5, 3, 0, 7, 4, 6)]
    inputs = {"camera_mono": rng.uniform(20, 235, (FRAMES, 12, 70, 3)).astype(np.float32),
              "radar_bev": rng.uniform(20, 235, (FRAMES, 16, 107, 6)).astype(np.float32),
              "radar_front": rng.uniform(20, 235, (FRAMES, 5, 107, 6)).astype(np.float32)}
    return samples, inputs


def _loader(cuts, zero=()):
    """[(data, labels)] over frames [a, b) per cut; ``zero``: views zeroed with torch (the dataset's dropout)."""
    samples, inputs = _split()
    out = []
    for a, b in cuts:
        data = {k: torch.from_numpy(v[a:b]).to(DEV) for k, v in inputs.items()}
        for k in zero:
            data[k] = torch.zeros_like(data[k])
        data["frame"] = torch.arange(a, b, device=DEV)
        labels = [dict({k: torch.from_numpy(s[k]).to(DEV) for k in ("gt_center", "gt_size", "gt_angle", "gt_class")},
                       description=torch.tensor([f % 8, f % 2, f % 7], device=DEV)) for f, s in zip(range(a, b), samples[a:b])]
        out.append((data, labels))
    return out


class _InputDrivenModel(torch.nn.Module):
    """The prepared queries of a frame, moved by what the model sees: the camera frame scales the class logits of the object
    classes, the radar maps shift the centres.  Per-sample sums over whole tensors of one sample: their bits do not depend on
    how many samples the batch holds."""

    def __init__(self):
        super().__init__()
        samples, _ = _split()
        self.base = {k: torch.from_numpy(np.stack([s[src] for s in samples])).to(DEV)
                     for k, src in (("class", "cls"), ("center", "center"), ("size", "size"), ("angle", "angle"))}
        self.calls, self.outputs, self.seen = 0, [], []

    def forward(self, data):
        self.calls += 1
        f = data["frame"]
        B = f.shape[0]
        cam = torch.stack([data["camera_mono"][b].sum() for b in range(B)]) / float(12 * 70 * 3 * 255)
        rad = torch.stack([data["radar_bev"][b].sum() / float(16 * 107 * 6 * 255) + data["radar_front"][b].sum() / float(5 * 107 * 6 * 255)
                           for b in range(B)])
        cls = self.base["class"][f].clone()
        cls[:, :, 1:] = cls[:, :, 1:] * (0.25 + cam)[:, None, None]
        center = self.base["center"][f] + (rad - 1.0)[:, None, None] * 0.4
        out = {"class": cls, "center": center, "size": self.base["size"][f], "angle": self.base["angle"][f]}
        self.outputs.append(out)
        self.seen.append({k: data[k] for k in ("camera_mono", "radar_bev", "radar_front")})
        return out


def _metric(output, labels):
    return {"score": output["class"][:, :, 1:].sum(), "shift": output["center"].sum()}


def _evaluator(robustness=True, exporter=None):
    from dpft_amd.evaluation import DataParallelEvaluator
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.evaluation.robustness import RobustnessSuite
    return DataParallelEvaluator(metric=_metric, exporter=exporter, device=DEV, dataset_ap=DatasetAP(C4, groups=["weather"], **AP),
                                 robustness=RobustnessSuite(SPEC) if robustness else None)


@functools.lru_cache(maxsize=None)
def _full_run():
    exported = []
    ev = _evaluator(exporter=lambda output, labels, step, dst: exported.append((output, step)))
    model = _InputDrivenModel()
    scalars = ev.evaluate_one_epoch(0, model, _loader([(0, 4), (4, 6)]), dst="unused", shard_start=0)
    return scalars, model, exported


def _same(a, b):
    return a == b or (a != a and b != b)                           # (NaN: a class without ground truth in a group)


def test_keys_calls_and_the_exporter():
    scalars, model, exported = _full_run()
    K = len(CONDITIONS)
    assert model.calls == 2 * (1 + K)
    clean = {k for k in scalars if "/cond=" not in k}
    assert {"score", "shift", "mAP_3d@0.5"} <= clean
    grouped = sorted(k for k in clean if k.startswith("mAP_3d@0.5/weather="))
    assert grouped
    for name in CONDITIONS:
        assert {k for k in scalars if k.endswith(f"/cond={name}")} == {f"{k}/cond={name}" for k in clean}, name
    assert f"{grouped[0]}/cond=camera_off" in scalars             # the condition comes after the group suffix
    # the exporter saw the two clean outputs, numbered by their first frame, and nothing else
    assert [(o is model.outputs[i], step) for (o, step), i in zip(exported, (0, 1 + K))] == [(True, 0), (True, 4)]
    assert len(exported) == 2
    # the clean pass got the loader's own tensors; every condition but "nothing" a changed view
    loader = _loader([(0, 4), (4, 6)])
    for i, (data, _) in zip((0, 1 + K), loader):
        for k, v in model.seen[i].items():
            assert torch.equal(v, data[k])
    assert any(scalars[k] != scalars[f"{k}/cond=camera_off"] for k in clean if k.startswith("mAP") and scalars[k] == scalars[k])


def test_a_condition_of_zero_severity_is_the_clean_table_bit_for_bit():
    scalars, model, _ = _full_run()
    clean = [k for k in scalars if "/cond=" not in k]
    for k in clean:
        assert _same(scalars[k], scalars[f"{k}/cond=nothing"]), k
    names = list(CONDITIONS)
    seen_nothing = model.seen[1 + names.index("nothing")]
    for k, v in model.seen[0].items():
        assert seen_nothing[k] is v, k                              # no launch: the very same tensors


@pytest.mark.parametrize("name,zero", [("camera_off", ("camera_mono",)), ("radar_off", ("radar_bev", "radar_front"))])
def test_off_conditions_equal_a_loader_zeroed_with_torch(name, zero):
    scalars, _, _ = _full_run()
    ev = _evaluator(robustness=False)
    want = ev.evaluate_one_epoch(0, _InputDrivenModel(), _loader([(0, 4), (4, 6)], zero=zero), shard_start=0)
    assert want and not any("/cond=" in k for k in want)
    for k, v in want.items():
        assert _same(v, scalars[f"{k}/cond={name}"]), (k, v, scalars[f"{k}/cond={name}"])
    assert any(want[k] != scalars[k] for k in want if want[k] == want[k])


def test_one_rank_and_two_played_ranks_give_the_same_condition_tables():
    """Ranks 0 and 1 of 2 take frames [0, 3) and [3, 6) in batches cut elsewhere than the one-rank run's; their per-condition
    accumulators merged give the one-rank tables bit for bit (noise keys hang on the global frame index alone), and every
    degraded tensor a frame's forward saw has the bits it had in the one-rank run."""
    scalars, model, _ = _full_run()
    K, names = len(CONDITIONS), list(CONDITIONS)
    merged, seen = {}, {}
    for rank, (cuts, start) in enumerate(([[(0, 2), (2, 3)], 0], [[(3, 6)], 3])):
        ev = _evaluator()
        m = _InputDrivenModel()
        ev.evaluate_one_epoch(0, m, _loader(cuts), shard_start=start, rank=rank, world=2)
        for j, (a, b) in enumerate(cuts):
            for c, name in enumerate(names):
                for k, v in m.seen[j * (1 + K) + 1 + c].items():
                    for f in range(a, b):
                        seen[(name, k, f)] = v[f - a]
        for name, ap in ev.condition_ap.items():
            if name in merged:
                merged[name].merge(ap)
            else:
                merged[name] = ap
    for j, (a, b) in enumerate([(0, 4), (4, 6)]):
        for c, name in enumerate(names):
            for k, v in model.seen[j * (1 + K) + 1 + c].items():
                for f in range(a, b):
                    assert torch.equal(seen[(name, k, f)], v[f - a]), (name, k, f)
    for name in names:
        table = merged[name].scalars()
        assert table
        for k, v in table.items():
            assert _same(v, scalars[f"{k}/cond={name}"]), (name, k)
    noisy = names.index("noisy")
    assert not torch.equal(model.seen[1 + noisy]["camera_mono"], model.seen[0]["camera_mono"])


def test_without_the_key_nothing_changes():
    ev = _evaluator(robustness=False)
    model = _InputDrivenModel()
    scalars = ev.evaluate_one_epoch(0, model, _loader([(0, 4), (4, 6)]), shard_start=0)
    assert model.calls == 2 and not any("/cond=" in k for k in scalars) and ev.robustness is None
    full, _, _ = _full_run()
    for k, v in scalars.items():
        assert _same(v, full[k]), k                                 # the clean numbers do not move when conditions ride along
