"""The views of ``TestTimeAugmentation.views``: built by the launches of dpft_amd/data/augment.py on the preprocessed batch, without a
resize or a rescaling.  A flip-only view is the mirrored copy of every camera frame and radar map bit for bit (whatever the floats:
-0, inf and NaN included), and its own inverse."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch():
    rng = np.random.default_rng(77)
    cam = rng.uniform(0, 255, (2, 6, 10, 3)).astype(np.float32)
    cam[0, 0, 0, 0], cam[0, 1, 3, 1], cam[1, 2, 9, 2], cam[1, 5, 4, 0] = -0.0, np.inf, np.nan, -3.5
    rad = rng.uniform(0, 255, (2, 5, 8, 4)).astype(np.float32)
    rad[0, 0, 7, 3], rad[1, 4, 0, 0] = -0.0, -np.inf
    data = {"camera_mono": torch.from_numpy(cam), "radar_bev": torch.from_numpy(rad), "frame": torch.arange(2)}
    for k, (H, W) in (("camera_mono", (720, 1280)), ("radar_bev", (256, 107))):
        data[f"{k}_shape"] = torch.tensor([[H, W, 3]] * 2, dtype=torch.int64)
        data[f"label_to_{k}_t"] = torch.from_numpy(rng.normal(0, 1, (2, 4, 4)).astype(np.float32))
        data[f"label_to_{k}_p"] = torch.from_numpy(rng.normal(0, 100, (2, 3 if k == "radar_bev" else 4, 4)).astype(np.float32))
    return {k: v.to(DEV) for k, v in data.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tta(*views):
    from dpft_amd.evaluation.tta import TestTimeAugmentation
    return TestTimeAugmentation(views=list(views))


def test_view_0_is_the_batch_itself_and_a_flip_view_is_the_mirrored_copy_bit_for_bit():
    data = _batch()
    views = _tta({"flip": True}).views(data)
    assert len(views) == 2 and views[0] is data
    v = views[1]
    assert v is not data and list(v) == list(data)
    for k in ("camera_mono", "radar_bev"):
        assert v[k].dtype == torch.float32 and v[k].shape == data[k].shape and v[k] is not data[k]
        assert torch.equal(_bits(v[k]), _bits(data[k].flip(2))), k
    assert v["frame"] is data["frame"] and v["camera_mono_shape"] is data["camera_mono_shape"]


def test_the_flip_view_applied_twice_restores_the_bits():
    data = _batch()
    tta = _tta({"flip": True})
    twice = tta.views(tta.views(data)[1])[1]
    for k in ("camera_mono", "radar_bev"):
        assert torch.equal(_bits(twice[k]), _bits(data[k])), k
    for k in ("label_to_camera_mono_t", "label_to_camera_mono_p", "label_to_radar_bev_t", "label_to_radar_bev_p"):
        # (F T F and M P F with M = [[-1, ., W], ...] are involutions up to the rounding of W - (W - x); T only changes signs)
        if k.endswith("_t"):
            assert torch.equal(_bits(twice[k]), _bits(data[k])), k
        else:
            assert torch.allclose(twice[k], data[k], rtol=0, atol=0.5), k      # (W |P[2]| ~ 1280 * 400: an fp32 ulp of 0.03)


@pytest.mark.parametrize("spec", [{"flip": True}, {"zoom": 1.1}, {"flip": True, "zoom": 0.9}])
def test_the_matrices_are_those_of_augment_geometry_for_the_same_parameters(spec):
    from dpft_amd.data import augment as A
    data = _batch()
    v = _tta(spec).views(data)[1]
    params = [A.SampleParams(flip=spec.get("flip", False), zoom=spec.get("zoom", 1.0))] * 2
    want, _ = A.augment_geometry([(data[f"label_to_{k}_t"], data[f"label_to_{k}_p"], data[f"{k}_shape"], k == "camera_mono")
                                  for k in ("camera_mono", "radar_bev")], None, params)
    for k, (t, p) in zip(("camera_mono", "radar_bev"), want):
        assert torch.equal(_bits(v[f"label_to_{k}_t"]), _bits(t)) and torch.equal(_bits(v[f"label_to_{k}_p"]), _bits(p)), k
        assert v[f"label_to_{k}_p"] is not data[f"label_to_{k}_p"]
    if spec.get("zoom", 1.0) != 1.0:
        cam = A.augment_camera(data["camera_mono"], None, params)
        assert torch.equal(_bits(v["camera_mono"]), _bits(cam)) and v["camera_mono"].shape == data["camera_mono"].shape


def test_a_zoom_view_leaves_the_radar_tensors_the_same_objects():
    data = _batch()
    v = _tta({"zoom": 1.1}).views(data)[1]
    assert v["radar_bev"] is data["radar_bev"] and v["camera_mono"] is not data["camera_mono"]
    assert not torch.equal(_bits(v["camera_mono"]), _bits(data["camera_mono"]))
    # the radar matrices of an unflipped sample are copies of the same bits
    assert torch.equal(_bits(v["label_to_radar_bev_p"]), _bits(data["label_to_radar_bev_p"]))
    assert torch.equal(_bits(v["label_to_radar_bev_t"]), _bits(data["label_to_radar_bev_t"]))


def test_three_views_and_a_batch_without_matrices():
    data = {k: v for k, v in _batch().items() if not k.startswith("label_to_")}
    views = _tta({"flip": True}, {"zoom": 1.1}, {"flip": True, "zoom": 0.9}).views(data)
    assert len(views) == 4 and views[0] is data and all(list(v) == list(data) for v in views)
    assert torch.equal(_bits(views[1]["radar_bev"]), _bits(views[3]["radar_bev"])) and views[2]["radar_bev"] is data["radar_bev"]
