"""End to end: the augmenting ``GpuPreprocessor`` moves image, radar maps, matrices and labels TOGETHER -- what the decoder
samples at the projected ground-truth centres is the same before and after -- and the loader and the trainer take it."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

CAM, BEV, FRONT = (48, 64, 3), (16, 107, 6), (8, 107, 6)        # raw (H, W, C); the camera is resized to 24 x 32
VIEWS = ("camera_mono", "radar_bev", "radar_front")
PARAMS = [dict(flip=True), dict(zoom=0.8, shift=(0.05, -0.05)), dict(flip=True, zoom=1.25, shift=(-0.05, 0.04)),
          dict(zoom=1.25, shift=(0.05, 0.05)), dict()]
Q = 6


def _ramp(H, W, coef, lo):
    """(H,W,C) affine ramps value = alpha_c x + beta_c y + gamma_c; ``coef`` rows (alpha, beta, gamma)."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return torch.stack([a * x + b * y + c + lo for a, b, c in coef], -1).float()


CAM_COEF = [(2.0, 1.5, 10.0), (-1.0, 2.0, 100.0), (0.5, -1.25, 90.0)]
RAD_COEF = [(0.5, 1.0, 10.0), (-0.25, 0.5, 40.0), (0.125, -1.0, 30.0), (0.75, 0.25, 5.0), (-0.5, -0.5, 70.0), (0.25, 2.0, 20.0)]


def _scene(B):
    """Ramp canvases, matrices that put every centre into the central 60 % of every view, labels with Q boxes each."""
    g = torch.Generator().manual_seed(12)
    batch = {"camera_mono": _ramp(*CAM[:2], CAM_COEF, 0.0).repeat(B, 1, 1, 1),
             "radar_bev": _ramp(*BEV[:2], RAD_COEF, 100.0).repeat(B, 1, 1, 1),          # dB inside (100, 200): never clipped
             "radar_front": _ramp(*FRONT[:2], RAD_COEF, 100.0).repeat(B, 1, 1, 1)}
    assert 0 <= float(batch["camera_mono"].min()) and float(batch["camera_mono"].max()) <= 255
    for k in ("radar_bev", "radar_front"):
        assert 100 < float(batch[k].min()) and float(batch[k].max()) < 200
    for k, s in zip(VIEWS, (CAM, BEV, FRONT)):
        batch[f"{k}_shape"] = torch.tensor([list(s)] * B, dtype=torch.int64)
    t = torch.eye(4).repeat(B, 1, 1)
    t[:, :3, 3] = torch.tensor([0.3, 0.1, 0.05]) + torch.rand(B, 3, generator=g) * 0.05
    batch["label_to_camera_mono_t"] = torch.zeros(B, 4, 4)
    batch["label_to_camera_mono_p"] = torch.tensor([[32.0, -30, 0, 0], [24, 0, -30, 0], [1, 0, 0, 0], [0, 0, 0, 1]]).repeat(B, 1, 1)
    batch["label_to_radar_bev_t"] = t
    batch["label_to_radar_bev_p"] = torch.tensor([[0, -1.0, 0, 53.5], [16 / 80.0, 0, 0, 0], [0, 0, 0, 1]]).repeat(B, 1, 1)
    batch["label_to_radar_front_t"] = t.clone()
    batch["label_to_radar_front_p"] = torch.tensor([[0, -1.0, 0, 53.5], [0, 0, 1.0, 4], [0, 0, 0, 1]]).repeat(B, 1, 1)
    labels = []
    for _ in range(B):
        x = 20 + torch.rand(Q, generator=g) * 30
        c = torch.stack((x, x * (torch.rand(Q, generator=g) - 0.5), torch.rand(Q, generator=g) * 1.2 - 0.6), -1)
        yaw = torch.rand(Q, generator=g) * 6.28 - 3.14
        labels.append({"gt_center": c, "gt_size": torch.ones(Q, 3), "gt_angle": torch.stack((yaw.sin(), yaw.cos()), -1),
                       "gt_class": torch.tensor([[0.0, 1.0]]).repeat(Q, 1)})
    return batch, labels


def _sampled(batch, labels):
    """{view: (B,Q,C)}: the level-0 input of every view sampled at the reference points of the ground-truth centres -- the
    project's own device rule for the points (train_fused.reference_points), grid_sample(align_corners=False) for the read."""
    from dpft_amd.models.fusers import train_fused as tf
    proj = tf._Proj([(batch[f"label_to_{k}_t"], batch[f"label_to_{k}_p"]) for k in VIEWS], [batch[f"{k}_shape"] for k in VIEWS],
                    [False, True, True])
    center = torch.stack([l["gt_center"] for l in labels])
    refs = tf.reference_points(proj, center)                                     # (V,B,Q,2) = (u / W, v / H)
    out = {}
    for v, k in enumerate(VIEWS):
        grid = (refs[v] * 2 - 1)[:, :, None, :]                                  # (B,Q,1,2)
        out[k] = F.grid_sample(batch[k].permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros",
                               align_corners=False)[..., 0].permute(0, 2, 1)
    return out, refs


def test_image_matrices_and_labels_move_together():
    """Camera canvases and radar maps hold affine ramps (bilinear interpolation reproduces a ramp away from the borders), the
    centres project into the central 60 % of every view, so they stay inside every warped image (zoom in [0.8, 1.25], shift
    <= 0.05: 0.3 * 1.25 + 0.05 < 0.5) -- checked here in fp64 first, no point is left out.  For flip, zoom and flip + zoom:
    what is read at the augmented centres from the augmented inputs equals what is read at the original centres from the
    plain inputs, within 8 ulp32(255) + 8 ulp32(max(W, H)) D with D the ramp's step |d/dx| + |d/dy| per pixel of the map
    that is sampled (the larger of the two sets).  Largest observed error on gfx950: 0.042 of the bound on the camera, 0.055 on
    the radar maps."""
    from dpft_amd.data import GpuPreprocessor
    from dpft_amd.data.augment import SampleParams
    B = len(PARAMS)
    batch, labels = _scene(B)
    for b in range(B):                                                           # fp64, on the host: central 60 % of every view
        for k, s in zip(VIEWS, (CAM, BEV, FRONT)):
            ref = R.reference_points(labels[b]["gt_center"].double().numpy(), batch[f"label_to_{k}_t"][b].double().numpy(),
                                     batch[f"label_to_{k}_p"][b].double().numpy(), s[:2])
            assert ref.min() >= 0.2 and ref.max() <= 0.8, (k, b, ref.min(), ref.max())
            q = PARAMS[b]
            m = R.camera_map(1.0, 1.0, q.get("flip", False), q.get("zoom", 1.0), q.get("shift", (0.0, 0.0))) \
                if k == "camera_mono" else R.radar_map(1.0, q.get("flip", False))
            moved = np.stack([m[0] * ref[:, 0] + m[1], m[2] * ref[:, 1] + m[3]], 1)
            assert moved.min() > 0.05 and moved.max() < 0.95, (k, b)
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    dlabels = [{k: v.to(DEV) for k, v in l.items()} for l in labels]
    plain = GpuPreprocessor(image_size=(24, 32))(dbatch)
    pre = GpuPreprocessor(image_size=(24, 32), augment={"flip": 0.5})
    abatch, alabels = pre._augmented(dbatch, dlabels, params=[SampleParams(**q) for q in PARAMS])
    assert abatch["camera_mono"].shape == (B, 24, 32, 3)
    want, refs0 = _sampled(plain, dlabels)
    got, refs1 = _sampled(abatch, alabels)
    assert float(refs0.min()) >= 0.2 and float(refs0.max()) <= 0.8 and float(refs1.min()) > 0.05 and float(refs1.max()) < 0.95
    worst = {}
    for k, s, coef in zip(VIEWS, (CAM, BEV, FRONT), (CAM_COEF, RAD_COEF, RAD_COEF)):
        H, W = s[:2]
        unit = 1.0 if k == "camera_mono" else 2.55                               # dB -> [0, 255]
        step = np.array([(abs(a) + abs(b)) * unit for a, b, _ in coef])          # per source pixel
        for b, q in enumerate(PARAMS):
            per_px = 2.0 / q.get("zoom", 1.0) if k == "camera_mono" else 1.0    # source pixels per pixel of the sampled map
            D = step * max(per_px, 2.0 if k == "camera_mono" else 1.0)
            bound = 8 * R.ulp32(255) + 8 * R.ulp32(max(W, H)) * D
            err = (got[k][b] - want[k][b]).abs().double().cpu().numpy()         # (Q,C)
            worst[k] = max(worst.get(k, 0.0), float((err / bound).max()))
            assert np.all(err <= bound), (k, b, float((err / bound).max()))
        # and the closed form: the ramp at the original reference point (fp64), loosely -- guards against both sets being wrong
        for b in range(B):
            ref = R.reference_points(labels[b]["gt_center"].double().numpy(), batch[f"label_to_{k}_t"][b].double().numpy(),
                                     batch[f"label_to_{k}_p"][b].double().numpy(), (H, W))
            x, y = ref[:, 0] * W - 0.5, ref[:, 1] * H - 0.5
            lo = 0.0 if k == "camera_mono" else 100.0
            exp = np.stack([a * x + bb * y + c + lo for a, bb, c in coef], -1)
            exp = exp if k == "camera_mono" else (exp - 100.0) / 100.0 * 255.0
            assert np.abs(got[k][b].double().cpu().numpy() - exp).max() < 1e-2, (k, b)
    print("largest error / bound per view:", {k: round(v, 3) for k, v in worst.items()})
    # the flipped samples really flipped: labels and the azimuth axis of the maps
    assert torch.equal(alabels[0]["gt_center"][:, 1], -dlabels[0]["gt_center"][:, 1])
    assert torch.equal(abatch["radar_bev"][0], torch.flip(plain["radar_bev"][0], [1]))
    assert torch.equal(abatch["camera_mono"][4], plain["camera_mono"][4]) and torch.equal(alabels[4]["gt_center"], dlabels[4]["gt_center"])


RAW = {"camera_mono": (36, 64, 3), "radar_bev": (32, 43, 6), "radar_front": (9, 43, 6)}
SPEC = {"flip": 0.5, "camera": {"zoom": [0.9, 1.1], "shift": 0.05, "brightness": 0.2, "contrast": 0.2, "channel": 0.05},
        "radar": {"gain_db": 3.0}, "seed": 3}


def _loader_config(augment):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["train"]["batch_size"] = 2
    cfg["train"]["shuffle"] = False
    cfg["data"]["image_size"] = 24
    cfg["computing"] = dict(cfg.get("computing", {}), workers=0)
    if augment:
        cfg["train"]["augment"] = SPEC
    return cfg


def test_loader_passes_labels_and_is_reproducible():
    """``load_listed`` + ``PrefetchLoader`` on raw synthetic samples with the key set: batches arrive as (batch, labels) with
    flipped labels where the frames flipped, the same seed gives the same bits twice, another epoch other flips; without the
    key the batch is today's."""
    from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset, listed_collating, load_listed
    ds = SyntheticRawDataset(8, seed=2, raw_shapes=RAW)
    cfg = _loader_config(True)
    pre = GpuPreprocessor.from_config(cfg, augment=True)
    assert pre.augments
    loader, sampler = load_listed(ds, cfg, device="cuda:0", preprocessor=pre, seed=1)

    def epoch(e):
        sampler.set_epoch(e)
        out = list(loader)
        torch.cuda.synchronize()
        return out
    first, again, other = epoch(0), epoch(0), epoch(1)
    assert len(first) == 4
    for (b0, l0), (b1, l1) in zip(first, again):
        assert set(b0) == set(b1)
        for k in b0:
            assert torch.equal(b0[k], b1[k]), k
        for x, y in zip(l0, l1):
            for k in x:
                assert torch.equal(x[k], y[k]), k

    def flips(batches):
        out = []
        for i, (_, lab) in enumerate(batches):
            for j, l in enumerate(lab):
                orig = ds[2 * i + j][1]["gt_center"]
                flipped = torch.equal(l["gt_center"][:, 1].cpu(), -orig[:, 1])
                assert flipped or torch.equal(l["gt_center"].cpu(), orig)
                assert torch.equal(l["gt_size"].cpu(), ds[2 * i + j][1]["gt_size"])
                out.append(flipped)
        return out
    f0, f1 = flips(first), flips(other)
    assert f0 == flips(again) and f0 != f1 and any(f0) and not all(f0)
    batch, labels = first[0]
    assert batch["camera_mono"].shape == (2, 24, 42, 3) and batch["camera_mono"].dtype == torch.float32
    assert batch["camera_mono_shape"].tolist() == [[36, 64, 3]] * 2
    assert all(v.is_cuda for v in labels[0].values())
    # the flip reached the radar map and the matrices of the same samples
    host_in, _ = listed_collating([ds[i] for i in range(2)])
    for j in range(2):
        p0, p1 = host_in["label_to_radar_bev_p"][j], batch["label_to_radar_bev_p"][j].cpu()
        want = p0.clone()
        if f0[j]:
            want[0] = -p0[0] + 43.0 * p0[2]
            want[:, 1] = -want[:, 1]
        assert torch.equal(p1, want), j
    # key absent: exactly the plain pipeline, and plain batches
    cfg0 = _loader_config(False)
    pre0 = GpuPreprocessor.from_config(cfg0, augment=True)
    assert not pre0.augments
    loader0, _ = load_listed(ds, cfg0, device="cuda:0", preprocessor=pre0, seed=1)
    b_plain, l_plain = next(iter(loader0))
    direct = GpuPreprocessor(image_size=24)({k: v.cuda() for k, v in host_in.items()})
    assert set(direct) == set(b_plain)
    for k in direct:
        assert torch.equal(direct[k], b_plain[k]), k
    assert torch.equal(l_plain[0]["gt_center"].cpu(), ds[0][1]["gt_center"])


def test_trainer_takes_an_augmented_batch():
    """Two ``DataParallelTrainer.train_step``s on an augmented batch at the smallest configuration the trainer tests use: the
    fused training path accepts the augmented matrices and labels."""
    from dpft_amd.data import GpuPreprocessor
    from dpft_amd.models import build
    from dpft_amd.synthetic import make_batch, make_labels
    from dpft_amd.training.trainer import DataParallelTrainer
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["model"]["backbones"]["camera_mono"]["name"] = "ResNet50"
    cfg["model"]["fuser"]["dropout"] = 0.0
    shapes = {"camera_mono": (96, 160, 3), "radar_bev": (128, 43, 6), "radar_front": (37, 107, 6)}
    batch = make_batch(cfg["model"]["inputs"], 2, seed=9, shapes=shapes, device=DEV)
    labels = make_labels(2, seed=9, device=DEV)
    pre = GpuPreprocessor(image_size=None, scale=False, augment=dict(SPEC, flip=1.0))
    abatch, alabels = pre(batch, labels)
    assert torch.equal(alabels[0]["gt_center"][:, 1], -labels[0]["gt_center"][:, 1])
    assert not abatch["label_to_camera_mono_t"].any() and abatch["label_to_radar_bev_t"].any()
    torch.manual_seed(0)
    tr = DataParallelTrainer(build("dprt", cfg), cfg, torch.device(DEV))
    for _ in range(2):
        loss, _ = tr.train_step(abatch, alabels)
        assert torch.isfinite(loss)
