"""Host side of the evaluator's robustness conditions (dpft_amd/evaluation/robustness.py): parsing, key naming, noise keys.
No GPU."""
import copy

import pytest

DOC = {"conditions": {"camera_off": {"camera": "off"}, "radar_off": {"radar": "off"},
                      "fog": {"camera": {"haze": 0.6, "blur": 2.0}},
                      "noisy": {"camera": {"noise": 15}, "radar": {"noise": 8}},
                      "sector": {"radar": {"azimuth_mask": [[0.4, 0.6]]}}},
       "seed": 0}


def test_suite_parses_the_documented_form():
    from dpft_amd.evaluation.robustness import RobustnessSuite
    s = RobustnessSuite(DOC)
    assert s.names == ["camera_off", "radar_off", "fog", "noisy", "sector"] and s.seed == 0
    cams, rads = s.params("camera_off", 10, 3)
    assert all(c.off for c in cams) and all(r.neutral for r in rads) and len(cams) == len(rads) == 3
    cams, rads = s.params("radar_off", 0, 2)
    assert all(c.neutral for c in cams) and all(r.off for r in rads)
    cams, rads = s.params("fog", 0, 1)
    assert (cams[0].haze, cams[0].blur, cams[0].noise, cams[0].erase) == (0.6, 2.0, 0.0, []) and rads[0].neutral
    cams, rads = s.params("noisy", 0, 1)
    assert (cams[0].noise, rads[0].noise, rads[0].channels) == (15.0, 8.0, None)
    cams, rads = s.params("sector", 0, 1)
    assert cams[0].neutral and rads[0].azimuth == [(0.4, 0.6)] and rads[0].rows == []
    full = RobustnessSuite({"conditions": {"x": {"camera": {"erase": [[0.1, 0.2, 0.3, 0.4]], "airlight": [1, 2, 3]},
                                                 "radar": {"range_mask": [[0, 0.1]], "channels": [0, 1]}}}})
    cams, rads = full.params("x", 0, 1)
    assert cams[0].erase == [(0.1, 0.2, 0.3, 0.4, (0.0,) * 4)] and rads[0].rows == [(0.0, 0.1)] and rads[0].channels == (0, 1)


def _with(name, cond, **top):
    return dict({"conditions": {name: cond}}, **top)


@pytest.mark.parametrize("bad", [
    None, True, [], {}, {"conditions": {}}, {"conditions": []}, {"conditions": {"a": {}}, "seeds": 1},
    _with("a", {}, seed=1.5), _with("a", {}, seed=True), _with("a/b", {}), _with("a=b", {}), _with("", {}), _with("a b", {}),
    _with("a", "off"), _with("a", {"lidar": "off"}), _with("a", {"camera": "on"}), _with("a", {"camera": {"fog": 1}}),
    _with("a", {"camera": {"haze": 1.5}}), _with("a", {"camera": {"haze": [0, 0.5]}}), _with("a", {"camera": {"blur": 6}}),
    _with("a", {"camera": {"blur": -1}}), _with("a", {"camera": {"noise": "x"}}), _with("a", {"camera": {"noise": float("nan")}}),
    _with("a", {"camera": {"erase": [[0, 1, 0]]}}), _with("a", {"camera": {"erase": [[0.5, 0.4, 0, 1]]}}),
    _with("a", {"camera": {"erase": [[0, 1, 0, 1.5]]}}), _with("a", {"camera": {"erase": [[0, 1, 0, 1]] * 5}}),
    _with("a", {"camera": {"airlight": 256}}), _with("a", {"radar": 1}), _with("a", {"radar": {"gain": 1}}),
    _with("a", {"radar": {"noise": -1}}), _with("a", {"radar": {"azimuth_mask": [0.4, 0.6]}}),
    _with("a", {"radar": {"azimuth_mask": [[0.6, 0.4]]}}), _with("a", {"radar": {"azimuth_mask": [[0, 1]] * 5}}),
    _with("a", {"radar": {"range_mask": [[0, 2]]}}), _with("a", {"radar": {"channels": []}}),
    _with("a", {"radar": {"channels": [40]}}),
])
def test_parser_refuses_malformed_forms(bad):
    from dpft_amd.evaluation.robustness import parse_robustness
    with pytest.raises(ValueError, match="evaluate.robustness"):
        parse_robustness(bad)


def test_key_naming():
    from dpft_amd.evaluation.robustness import RobustnessSuite
    assert RobustnessSuite.scalar_key("mAP", "fog") == "mAP/cond=fog"
    assert RobustnessSuite.scalar_key("mAP_3d@0.5/weather=fog", "camera_off") == "mAP_3d@0.5/weather=fog/cond=camera_off"


def test_noise_keys_depend_on_seed_condition_and_global_frame_only():
    """A frame's key is the same whichever batch or rank it arrives in: (first_frame, batch) cuts of one split give one list."""
    from dpft_amd.evaluation.robustness import RobustnessSuite
    s = RobustnessSuite(DOC)

    def keys(cuts):
        out = []
        for first, n in cuts:
            cams, rads = s.params("noisy", first, n)
            assert [c.key for c in cams] == [r.key for r in rads]
            out += [c.key for c in cams]
        return out
    whole = keys([(0, 12)])
    assert len(set(whole)) == 12 and all(0 <= k < 1 << 64 for k in whole)
    assert keys([(0, 4), (4, 4), (8, 4)]) == whole == keys([(0, 5), (5, 1), (6, 6)])
    assert keys([(6, 3), (9, 3)]) == whole[6:]                      # the second of two ranks: its block starts at 6
    assert whole[3] == s.noise_key("noisy", 3)
    assert s.noise_key("noisy", 3) != s.noise_key("fog", 3)
    assert RobustnessSuite(dict(DOC, seed=1)).noise_key("noisy", 3) != whole[3]


def test_from_config_builds_a_suite_only_with_the_key():
    from dpft_amd.configs import load_config
    from dpft_amd.evaluation.evaluator import DataParallelEvaluator
    from dpft_amd.evaluation.robustness import RobustnessSuite
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["computing"] = dict(cfg.get("computing", {}), device="cpu")
    assert "robustness" not in cfg["evaluate"]
    ev = DataParallelEvaluator.from_config(cfg)
    assert ev.robustness is None
    assert RobustnessSuite.from_config(cfg) is None
    cfg["evaluate"]["robustness"] = DOC
    ev = DataParallelEvaluator.from_config(cfg)
    assert isinstance(ev.robustness, RobustnessSuite) and ev.robustness.names[0] == "camera_off"
    assert DataParallelEvaluator(device="cpu").robustness is None    # the new keyword is trailing and optional
    cfg["evaluate"]["robustness"] = {"conditions": {"a": {"camera": "dark"}}}
    with pytest.raises(ValueError, match="evaluate.robustness"):
        DataParallelEvaluator.from_config(cfg)


def test_eval_loader_refuses_a_corrupting_preprocessor():
    from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset, load_listed_eval
    pre = GpuPreprocessor(corrupt={"p": 1.0, "camera": {"off": 1.0}})
    with pytest.raises(ValueError, match="train.corrupt"):
        load_listed_eval(SyntheticRawDataset(2, seed=0), {"train": {"batch_size": 1}}, preprocessor=pre)
