"""``GpuPreprocessor`` with ``train.corrupt``: the degradation launches run after the plain or the augmented transforms, leave
labels and matrices alone, are reproducible from (seed, rank, epoch, ordinal), and never reach an evaluation preprocessor."""
import copy

import numpy as np
import pytest
import torch

from tests import corrupt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

RAW = {"camera_mono": (36, 64, 3), "radar_bev": (32, 43, 6), "radar_front": (9, 43, 6)}
AUG = {"flip": 0.5, "camera": {"zoom": [0.9, 1.1], "shift": 0.05, "brightness": 0.2}, "radar": {"gain_db": 3.0}, "seed": 3}
FULL = {"p": 1.0,
        "camera": {"blur": [0, 3], "haze": [0, 0.6], "noise": [0, 20],
                   "erase": {"n": [0, 3], "area": [0.02, 0.2], "aspect": [0.3, 3.3]}, "off": 0.05},
        "radar": {"noise": [0, 10], "azimuth_mask": {"n": [0, 2], "width": [1, 12]},
                  "range_mask": {"n": [0, 2], "width": [1, 24]}, "off": 0.05},
        "seed": 4}
VIEWS = ("camera_mono", "radar_bev", "radar_front")


def _batch(B=4):
    from dpft_amd.data import SyntheticRawDataset, listed_collating
    ds = SyntheticRawDataset(B, seed=2, raw_shapes=RAW)
    host, labels = listed_collating([ds[i] for i in range(B)])
    return {k: v.to(DEV) for k, v in host.items()}, [{k: v.to(DEV) for k, v in l.items()} for l in labels]


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_p_zero_is_the_preprocessor_without_the_key_plain_and_augmented():
    from dpft_amd.data import GpuPreprocessor
    batch, labels = _batch()
    off = dict(FULL, p=0.0)
    _same_bits(GpuPreprocessor(image_size=24, corrupt=off)(batch), GpuPreprocessor(image_size=24)(batch))
    a0, l0 = GpuPreprocessor(image_size=24, augment=AUG)(batch, labels)
    a1, l1 = GpuPreprocessor(image_size=24, augment=AUG, corrupt=off)(batch, labels)
    _same_bits(a0, a1)
    for x, y in zip(l0, l1):
        _same_bits(x, y)


def test_p_one_is_reproducible_and_leaves_labels_and_matrices_alone():
    from dpft_amd.data import GpuPreprocessor
    batch, labels = _batch()

    def run(seed, epoch, skip, augment=None):
        pre = GpuPreprocessor(image_size=24, augment=augment, corrupt=dict(FULL, seed=seed), rank=1)
        pre.set_epoch(epoch)
        for _ in range(skip):
            pre(batch, labels) if augment else pre(batch)
        return pre(batch, labels) if augment else pre(batch)
    first, again = run(4, 2, 1), run(4, 2, 1)
    _same_bits(first, again)
    plain = GpuPreprocessor(image_size=24)(batch)
    assert any(not torch.equal(first[k], plain[k]) for k in VIEWS)
    for other in (run(5, 2, 1), run(4, 3, 1), run(4, 2, 0)):
        assert any(not torch.equal(first[k], other[k]) for k in VIEWS)
    for k in batch:                                                # everything but the views: the very same objects
        if k not in VIEWS:
            assert first[k] is batch[k], k
    assert first["camera_mono"].shape == plain["camera_mono"].shape == (4, 24, 42, 3)
    # on the augmented path: matrices and labels have the bits of the augmentation alone
    (a0, l0), (a1, l1) = GpuPreprocessor(image_size=24, augment=AUG, rank=1)(batch, labels), run(4, 0, 0, augment=AUG)
    for k in a0:
        if k not in VIEWS:
            assert torch.equal(a0[k], a1[k]), k
    for x, y in zip(l0, l1):
        _same_bits(x, y)
    assert any(not torch.equal(a0[k], a1[k]) for k in VIEWS)


def test_given_parameters_reach_every_view_with_its_view_id():
    """The preprocessor's launches against the restatement on the plain transforms' outputs: camera_mono is view 0, radar_bev
    view 2, radar_front view 3 (positions in camera_keys + radar_keys); row bands act on the BEV map only."""
    from dpft_amd.data import GpuPreprocessor
    from dpft_amd.data.corrupt import CameraCorruption, RadarCorruption
    batch, _ = _batch(2)
    plain = {k: v.cpu().numpy() for k, v in GpuPreprocessor(image_size=24)(batch).items() if k in VIEWS}
    pre = GpuPreprocessor(image_size=24, corrupt=FULL)
    keys = [11, (1 << 63) + 5]
    cams = [CameraCorruption(noise=12.0, haze=0.3, key=keys[0]), CameraCorruption(key=keys[1])]
    rads = [RadarCorruption(noise=6.0, azimuth=[{"u": 0.5, "bins": 4}], rows=[(0.25, 0.5)], key=keys[0]),
            RadarCorruption(off=True, key=keys[1])]
    out = pre._corrupted(pre._plain(batch), params=(cams, rads))
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in VIEWS}
    assert np.array_equal(got["camera_mono"][0], R.camera(plain["camera_mono"][0], noise=12.0, haze=0.3, key=keys[0], view=0))
    assert np.array_equal(got["camera_mono"][1], plain["camera_mono"][1])
    a0 = int(0.5 * (43 - 4 + 1))
    assert np.array_equal(got["radar_bev"][0], R.radar(plain["radar_bev"][0], noise=6.0, azimuth=[(a0, a0 + 4)], rows=[(8, 16)],
                                                       key=keys[0], view=2))
    assert np.array_equal(got["radar_front"][0], R.radar(plain["radar_front"][0], noise=6.0, azimuth=[(a0, a0 + 4)],
                                                         key=keys[0], view=3))
    assert not got["radar_bev"][1].any() and not got["radar_front"][1].any()


def test_camera_off_and_radar_off_never_hit_the_same_sample():
    from dpft_amd.data import GpuPreprocessor
    B = 256
    batch = {"camera_mono": torch.rand(B, 4, 6, 3, device=DEV) * 200 + 20, "radar_bev": torch.rand(B, 3, 5, 2, device=DEV) * 200 + 20,
             "radar_front": torch.rand(B, 2, 5, 2, device=DEV) * 200 + 20}
    pre = GpuPreprocessor(image_size=None, scale=False, corrupt={"p": 1.0, "camera": {"off": 0.4}, "radar": {"off": 0.4}, "seed": 9})
    out = pre(batch)
    cam_off = ~out["camera_mono"].flatten(1).any(1)
    bev_off, front_off = ~out["radar_bev"].flatten(1).any(1), ~out["radar_front"].flatten(1).any(1)
    assert torch.equal(bev_off, front_off)                         # one sample's radar goes off in both maps
    assert not bool((cam_off & bev_off).any())
    n_cam, n_rad = int(cam_off.sum()), int(bev_off.sum())
    print("camera off", n_cam, "radar off", n_rad, "of", B)
    assert 60 < n_cam < 145 and 60 < n_rad < 145                   # 0.4 each: 102 +- 5 sigma
    keep = ~(cam_off | bev_off)
    assert torch.equal(out["camera_mono"][keep], batch["camera_mono"][keep])


def test_evaluation_preprocessors_ignore_the_key():
    from dpft_amd.configs import load_config
    from dpft_amd.data import GpuPreprocessor
    batch, _ = _batch()
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["data"]["image_size"] = 24
    base = GpuPreprocessor.from_config(cfg)(batch)
    cfg["train"]["corrupt"] = FULL
    pre = GpuPreprocessor.from_config(cfg)
    assert not pre.corrupts
    _same_bits(pre(batch), base)
    train = GpuPreprocessor.from_config(cfg, augment=True)
    assert train.corrupts and not train.augments
    assert any(not torch.equal(train(batch)[k], base[k]) for k in VIEWS)


def test_loader_carries_the_epoch_to_the_corrupt_sampler():
    """``load_listed`` + ``PrefetchLoader`` with the key alone (no augmentation): plain (batch, labels) pairs, the same bits for
    the same epoch, others for another epoch."""
    from dpft_amd.configs import load_config
    from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset, load_listed
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"].update(batch_size=2, shuffle=False, corrupt=FULL)
    cfg["data"]["image_size"] = 24
    cfg["computing"] = dict(cfg.get("computing", {}), workers=0)
    ds = SyntheticRawDataset(4, seed=2, raw_shapes=RAW)
    loader, sampler = load_listed(ds, cfg, device="cuda:0", preprocessor=GpuPreprocessor.from_config(cfg, augment=True), seed=1)

    def epoch(e):
        sampler.set_epoch(e)
        out = list(loader)
        torch.cuda.synchronize()
        return out
    first, again, other = epoch(0), epoch(0), epoch(1)
    assert len(first) == 2
    for (b0, l0), (b1, l1) in zip(first, again):
        _same_bits(b0, b1)
        assert torch.equal(l0[0]["gt_center"].cpu(), l1[0]["gt_center"].cpu())
    assert any(not torch.equal(first[0][0][k], other[0][0][k]) for k in VIEWS)
    assert torch.equal(first[0][1][0]["gt_center"].cpu(), ds[0][1]["gt_center"])
