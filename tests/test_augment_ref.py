"""Host side of the training augmentation (dpft_amd/data/augment.py) and the geometry contract it rests on, without a GPU:
the config key, the sampler, the preprocessor's call contract, and -- in fp64 -- that the augmented matrices and labels
project every centre to the augmented image position (tests/augment_ref.py restates the rules independently)."""
import copy

import numpy as np
import pytest
import torch

from tests import augment_ref as R

FULL = {"flip": 0.5,
        "camera": {"zoom": [0.9, 1.1], "shift": 0.05, "brightness": 0.2, "contrast": 0.2, "channel": 0.05},
        "radar": {"gain_db": 3.0}, "seed": None}


def test_parse_augment_accepts_the_documented_forms():
    from dpft_amd.data.augment import parse_augment
    off_cam = {"zoom": (1.0, 1.0), "shift": 0.0, "brightness": 0.0, "contrast": 0.0, "channel": 0.0}
    assert parse_augment(True) == {"flip": 0.5, "camera": off_cam, "radar": {"gain_db": 0.0}, "seed": None}
    assert parse_augment({"flip": 0.5}) == parse_augment(True)
    assert parse_augment({}) == dict(parse_augment(True), flip=0.0)
    got = parse_augment(FULL)
    assert got["flip"] == 0.5 and got["camera"]["zoom"] == (0.9, 1.1) and got["camera"]["shift"] == 0.05
    assert got["camera"]["brightness"] == 0.2 and got["camera"]["contrast"] == 0.2 and got["camera"]["channel"] == 0.05
    assert got["radar"] == {"gain_db": 3.0} and got["seed"] is None
    assert parse_augment({"flip": 1, "seed": 7})["seed"] == 7 and parse_augment({"flip": 0})["flip"] == 0.0
    assert parse_augment({"camera": {"zoom": [1.0, 1.0]}})["camera"]["zoom"] == (1.0, 1.0)


@pytest.mark.parametrize("bad", [
    False, None, 0.5, "on", [0.5], {"flips": 0.5}, {"flip": 1.5}, {"flip": -0.1}, {"flip": True}, {"flip": "0.5"},
    {"flip": float("nan")}, {"camera": {"zoom": [1.1, 0.9]}}, {"camera": {"zoom": [0.0, 1.0]}},
    {"camera": {"zoom": [-1.0, 1.0]}}, {"camera": {"zoom": 1.0}}, {"camera": {"zoom": [1.0]}}, {"camera": {"zooom": [1, 1]}},
    {"camera": {"shift": -0.1}}, {"camera": {"brightness": "a"}}, {"camera": [1]}, {"radar": {"gain": 3.0}},
    {"radar": {"gain_db": -1.0}}, {"radar": 3.0}, {"seed": 1.5}, {"seed": True}])
def test_parse_augment_rejects(bad):
    from dpft_amd.data.augment import parse_augment
    with pytest.raises(ValueError, match="train.augment"):
        parse_augment(bad)


def _config(augment=None, fov=None):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    if augment is not None:
        cfg["train"]["augment"] = augment
    if fov is not None:
        cfg["data"]["fov"] = fov
    return cfg


def test_from_config_takes_the_key_for_the_training_loader_only():
    from dpft_amd.data import GpuPreprocessor
    assert not GpuPreprocessor.from_config(_config()).augments
    assert not GpuPreprocessor.from_config(_config(), augment=True).augments                 # no key: nothing changes
    assert not GpuPreprocessor.from_config(_config(True)).augments                           # evaluation loaders
    pre = GpuPreprocessor.from_config(_config(FULL), augment=True, rank=3)
    assert pre.augments and pre.sampler.rank == 3 and pre.sampler.seed == 42                   # computing.seed
    assert GpuPreprocessor.from_config(_config(dict(FULL, seed=5)), augment=True).sampler.seed == 5
    with pytest.raises(ValueError, match="train.augment"):
        GpuPreprocessor.from_config(_config({"flipp": 1}), augment=True)


def test_flip_needs_a_symmetric_field_of_view():
    from dpft_amd.data import GpuPreprocessor
    sym = {"x": [0.0, 72.0], "y": [-6.4, 6.4], "z": [-2.0, 6.0], "azimuth": [-50, 50]}
    assert GpuPreprocessor.from_config(_config(True, sym), augment=True).augments
    assert GpuPreprocessor.from_config(_config(True, {"x": [0.0, 72.0]}), augment=True).augments      # no y / azimuth range
    for name, rng in (("y", [-6.4, 8.0]), ("azimuth", [-40, 50]), ("y", [0.0, 6.4])):
        with pytest.raises(ValueError, match=f"fov.{name}"):
            GpuPreprocessor.from_config(_config(True, dict(sym, **{name: rng})), augment=True)
    asym = dict(sym, y=[-6.4, 8.0])
    assert GpuPreprocessor.from_config(_config({"flip": 0.0, "radar": {"gain_db": 1.0}}, asym), augment=True).augments
    assert not GpuPreprocessor.from_config(_config(True, asym)).augments                     # not asked to augment: no check


def test_sampler_is_reproducible_from_seed_rank_epoch_and_ordinal():
    from dpft_amd.data.augment import N_DRAWS, AugmentSampler, parse_augment
    spec = parse_augment(FULL)

    def stream(seed, rank, epoch, n=3):
        s = AugmentSampler(spec, seed, rank)
        s.set_epoch(epoch)
        return [s.uniforms(4) for _ in range(n)]
    a, b = stream(1, 0, 0), stream(1, 0, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape == (4, N_DRAWS) and a[0].dtype == torch.float64
    assert not torch.equal(a[0], a[1])                                # the draws advance once per batch
    for other in (stream(2, 0, 0), stream(1, 1, 0), stream(1, 0, 1)):   # seed, rank and epoch each change the stream
        assert not any(torch.equal(x, y) for x in a for y in other)
    s = AugmentSampler(spec, 1, 0)
    s.set_epoch(0)
    s.uniforms(4)
    s.uniforms(4)
    s.set_epoch(0)                                                    # back to batch 0 of the epoch
    assert torch.equal(s.uniforms(4), a[0])
    assert AugmentSampler(parse_augment(dict(FULL, seed=9)), 1, 0).seed == 9      # the key's seed wins
    # the parameter objects of the same stream are equal too
    p, q = AugmentSampler(spec, 3, 1).draw(5), AugmentSampler(spec, 3, 1).draw(5)
    assert [(x.flip, x.a, x.bu, x.bv, x.gain, x.offset, x.delta_db) for x in p] == \
           [(x.flip, x.a, x.bu, x.bv, x.gain, x.offset, x.delta_db) for x in q]


def test_sampler_respects_the_ranges():
    from dpft_amd.data.augment import AugmentSampler, parse_augment
    spec = parse_augment(FULL)
    s = AugmentSampler(spec, 0, 0)
    flips = 0
    for _ in range(50):
        for p in s.draw(8):
            flips += p.flip
            assert 0.9 <= p.s <= 1.1 and p.a == (-p.s if p.flip else p.s)
            bu = 1.0 - p.bu if p.flip else p.bu
            assert abs(bu - (1 - p.s) / 2) <= 0.05 + 1e-15 and abs(p.bv - (1 - p.s) / 2) <= 0.05 + 1e-15
            contrast = 1.0 - p.offset / 127.5
            assert 0.8 - 1e-12 <= contrast <= 1.2 + 1e-12
            for g in p.gain:
                assert 0.8 * 0.95 - 1e-12 <= g / contrast <= 1.2 * 1.05 + 1e-12
            assert abs(p.delta_db) <= 3.0
    assert 120 < flips < 280                                          # 400 draws at p = 0.5: 10 sigma = 100
    never = AugmentSampler(parse_augment({"flip": 0.0}), 0, 0)
    always = AugmentSampler(parse_augment({"flip": 1.0}), 0, 0)
    for _ in range(10):
        for p in never.draw(8):                                       # everything off: the identity, exactly
            assert (p.flip, p.a, p.bu, p.s, p.bv, p.gain, p.offset, p.delta_db) == (False, 1, 0, 1, 0, [1.0] * 4, 0, 0)
        for p in always.draw(8):                                      # the pure flip: a = -1, b_u = W, exactly
            assert (p.flip, p.a, p.bu, p.s, p.bv, p.gain, p.offset, p.delta_db) == (True, -1, 1, 1, 0, [1.0] * 4, 0, 0)


def test_call_contract():
    """Off: the batch dict, as before.  On: (batch, labels), and a ValueError without labels -- raised before anything runs
    on the device (a flipped frame with unflipped labels is silent corruption)."""
    from dpft_amd.data import GpuPreprocessor
    batch = {"odometry": torch.arange(6.0).view(2, 3)}                # no view key: nothing for the device to do
    labels = [{"gt_center": torch.zeros(1, 3), "gt_angle": torch.zeros(1, 2)} for _ in range(2)]
    off = GpuPreprocessor(image_size=None)
    out = off(batch)
    assert isinstance(out, dict) and out is not batch and torch.equal(out["odometry"], batch["odometry"])
    assert isinstance(off(batch, labels), dict)                       # labels are ignored when nothing augments
    on = GpuPreprocessor(image_size=None, augment=True)
    assert on.augments and not off.augments
    got = on(batch, labels)
    assert isinstance(got, tuple) and len(got) == 2 and isinstance(got[0], dict) and len(got[1]) == 2
    with pytest.raises(ValueError, match="labels"):
        on(batch)
    with pytest.raises(ValueError, match="labels"):
        on({"camera_mono": torch.zeros(2, 4, 4, 3)})
    with pytest.raises(ValueError, match="train.augment"):
        GpuPreprocessor(augment={"flip": 2.0})


def test_evaluation_loader_refuses_an_augmenting_preprocessor():
    from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset
    from dpft_amd.data.loader import load_listed_eval
    cfg = _config()
    cfg["computing"]["workers"] = 0
    with pytest.raises(ValueError, match="never runs in evaluation"):
        load_listed_eval(SyntheticRawDataset(2), cfg, preprocessor=GpuPreprocessor(augment=True))


def test_worked_radar_example():
    """The fixed range-azimuth projection under a flip: row 0 becomes [0, -1, 0, 54], and with phi' = -phi the azimuth
    coordinate is u' = 107 - u -- not 106 - u: the index mirror x -> W - 1 - x and the sampler's - 0.5 make W - u exact."""
    P = np.array([[0, -1, 0, 53], [256 / 118.04, 0, 0, 0], [0, 0, 0, 1.0]])
    T = np.eye(4)
    T2, P2 = R.matrices(T, P, R.radar_map(107, flip=True), True)
    assert np.array_equal(P2, np.array([[0, -1, 0, 54], [256 / 118.04, 0, 0, 0], [0, 0, 0, 1.0]]))
    assert np.array_equal(T2, T)
    center = np.array([[20.0, 3.0, 0.5], [50.0, -6.0, -1.0], [7.0, 0.0, 0.0]])
    c2, _ = R.labels(center, np.zeros((3, 2)), True)
    u = R.reference_points(center, T, P, (256, 107))[:, 0] * 107
    u2 = R.reference_points(c2, T2, P2, (256, 107))[:, 0] * 107
    assert np.allclose(u2, 107 - u, rtol=0, atol=1e-12) and not np.allclose(u2, 106 - u, atol=0.5)
    # the sampled pixel: the mirrored map holds at index x what the original holds at W - 1 - x
    x, x2 = u - 0.5, u2 - 0.5
    assert np.allclose(x2, 107 - 1 - x, rtol=0, atol=1e-12)
    # the package's own (torch) rule agrees in fp64
    from dpft_amd.models.fusers.mpfusion import IMPFusion
    tt = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))[None]
    shape = torch.tensor([[256, 107]])
    got = IMPFusion.get_reference_points(tt(c2), tt(T2), tt(P2), shape)[0, :, 0] * 107
    ref = IMPFusion.get_reference_points(tt(center), tt(T), tt(P), shape)[0, :, 0] * 107
    assert torch.allclose(got, 107 - ref, rtol=0, atol=1e-12)


def _random_view(rs, kind):
    """(T, P, (H, W)): camera-like (4x4 P, all-zero T), radar-like (3x4 P, rigid T) and the two crossed.  The noise stays off
    the divisor row so that no divisor comes near 0 by accident (the zero divisor has cases of its own)."""
    if kind in ("camera", "camera_t"):
        H, W = 720, 1280
        P = np.array([[640.0, -560, 0, 0], [360, 0, -560, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
        if kind == "camera_t":                      # a 4x4 projection behind a non-zero T acts on (r, phi, roh)
            P = np.array([[0, -8.0, 0, 640], [0, 0, -8.0, 360], [0.01, 0, 0, 1], [0, 0, 0, 1]])
    else:
        H, W = 256, 107
        P = np.array([[0, -1.0, 0, 53], [256 / 118.04, 0, 0, 0], [0, 0, 0, 1]])
        if kind == "radar_zero_t":                  # a 3x4 projection with no transformation acts on (x, y, z)
            P = np.array([[40.0, -5, 0, 3], [20, 0, -5, 1], [1, 0, 0, 0.5]])
    P[:2] += rs.uniform(-0.05, 0.05, (2, 4))
    if kind in ("camera", "radar_zero_t"):
        T = np.zeros((4, 4))
    else:
        th = rs.uniform(-0.05, 0.05)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        T[:3, 3] = rs.uniform(-1, 1, 3)
    return T, P, (H, W)


CASES = [(False, 1.0, (0.0, 0.0)), (True, 1.0, (0.0, 0.0)), (False, 0.8, (0.05, -0.05)), (True, 1.25, (-0.05, 0.03)),
         (True, 0.9, (0.02, 0.05)), (False, 1.1, (-0.01, 0.0))]


def _check_identity(center, T, P, H, W, flip, zoom, shift, zero):
    m = R.camera_map(W, H, flip, zoom, shift)
    T2, P2 = R.matrices(T, P, m, flip)
    c2, _ = R.labels(center, np.zeros((len(center), 2)), flip)
    ref = R.reference_points(center, T, P, (H, W))
    got = R.reference_points(c2, T2, P2, (H, W))
    a, bu, s, bv = m
    want = np.stack([(a * ref[:, 0] * W + bu) / W, (s * ref[:, 1] * H + bv) / H], 1)
    want[zero] = np.stack([a * ref[zero, 0], s * ref[zero, 1]], 1)
    assert np.abs(got - want).max() <= 1e-12, (flip, zoom, shift, np.abs(got - want).max())
    # the package's rule in fp64 (it clips to [0, 1]) agrees
    from dpft_amd.models.fusers.mpfusion import IMPFusion
    tt = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))[None]
    own = IMPFusion.get_reference_points(tt(c2), tt(T2), tt(P2), torch.tensor([[H, W]]))[0].numpy()
    assert np.abs(own - np.clip(want, 0, 1)).max() <= 1e-12


@pytest.mark.parametrize("kind", ["camera", "camera_t", "radar", "radar_zero_t"])
def test_projection_identity_fp64(kind):
    """For every centre the un-clipped reference point of the AUGMENTED (centre, T, P) equals the augmented image position
    ((a u W + b_u) / W, (s v H + b_v) / H) of the original's reference point (u, v), to 1e-12 -- flipped and unflipped
    samples, zoom and shift of both signs, 3x4 and 4x4 P, zero and non-zero T."""
    rs = np.random.RandomState({"camera": 1, "camera_t": 2, "radar": 3, "radar_zero_t": 4}[kind])
    for flip, zoom, shift in CASES:
        T, P, (H, W) = _random_view(rs, kind)
        center = np.stack([rs.uniform(5, 70, 12), rs.uniform(-6, 6, 12), rs.uniform(-1.5, 2, 12)], 1)
        _check_identity(center, T, P, H, W, flip, zoom, shift, np.zeros(12, dtype=bool))


@pytest.mark.parametrize("with_t", [False, True])
def test_projection_identity_with_a_zero_divisor(with_t):
    """A point whose divisor w is 0 is left undivided by the rule, and the offset column of M multiplies that w: for those
    rows the statement is (a u, s v) -- no offset -- which is what is asserted; the other rows of the batch keep the full one."""
    rs = np.random.RandomState(5 + with_t)
    for flip, zoom, shift in CASES:
        center = np.stack([rs.uniform(5, 70, 8), rs.uniform(-6, 6, 8), rs.uniform(-1.5, 2, 8)], 1)
        zero = np.zeros(8, dtype=bool)
        zero[[1, 4]] = True
        if with_t:                                   # w = phi, 0 exactly for y = 0 (and -0 after the flip)
            T = np.eye(4)
            T[0, 3] = 0.5
            P = np.array([[3.0, -1, 0.5, 53], [2.0, 0.5, -3, 20], [0, 1, 0, 0], [0, 0, 0, 1]])
            center[zero, 1] = 0.0
        else:                                        # w = x
            T = np.zeros((4, 4))
            P = np.array([[40.0, -5, 0, 3], [20, 0, -5, 1], [1, 0, 0, 0]])
            center[zero, 0] = 0.0
        _check_identity(center, T, P, 48, 64, flip, zoom, shift, zero)


def test_zero_transformation_stays_zero_and_unflipped_samples_keep_their_labels():
    T2, P2 = R.matrices(np.zeros((4, 4)), np.eye(4), R.camera_map(10, 8, True, 1.0), True)
    assert not T2.any()
    c, a = R.labels([[1.0, 2.0, 3.0]], [[0.6, 0.8]], False)
    assert c.tolist() == [[1.0, 2.0, 3.0]] and a.tolist() == [[0.6, 0.8]]
    c, a = R.labels([[1.0, 2.0, 3.0]], [[0.6, 0.8]], True)
    assert c.tolist() == [[1.0, -2.0, 3.0]] and a.tolist() == [[-0.6, 0.8]]


def test_central_points_stay_inside_every_warped_image():
    """What the pipeline test relies on: a point in the central 60 % of a view stays inside the image for every zoom in
    [0.8, 1.25] and shift up to 0.05, flipped or not: 0.3 * 1.25 + 0.05 < 0.5."""
    assert 0.3 * 1.25 + 0.05 < 0.5
    for flip in (False, True):
        for zoom in (0.8, 1.0, 1.25):
            for sx in (-0.05, 0.05):
                a, bu, s, bv = R.camera_map(64, 48, flip, zoom, (sx, -sx))
                for u in (0.2 * 64, 0.8 * 64):
                    assert 0 < a * u + bu < 64
                for v in (0.2 * 48, 0.8 * 48):
                    assert 0 < s * v + bv < 48
